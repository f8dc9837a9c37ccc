"""The yardstick of the novel view (rslf_novel_view): numpy, written from the rule as include/rslf_hip.h states it, not from the
kernel -- no keys, no chunks, no scan over threads.  Stage A is view_warp_ref.warp; stage B has a vectorised form (running
maxima of the hit columns from either side) and a plain loop over the runs of a row; stage C is a loop over the walk,
vectorised over the pixels, every float operation a single binary32 one in the order the rule gives."""
import functools

import numpy as np

import view_warp_ref as wr
from consistency_ref import bits, planted, roundf

F = np.float32
NAMES = ("colour", "depth", "fill", "n_src", "err", "row_err", "row_cov")
PLANES = ("depth", "fill", "n_src", "row_cov")   # what a call without a volume can give
DTYPES = dict(colour=F, depth=F, fill=np.uint8, n_src=np.int32, err=F, row_err=np.float64, row_cov=np.int32)
HOLE, HIT, LEFT, RIGHT = 0, 1, 2, 3


def _z(d, nearer):
    return (d if nearer >= 0 else -d) + F(0)   # -0.0 + 0.0 = +0.0: the two zeros are one depth


def fill_vectorised(hit, dw, max_gap, nearer):
    """hit bool [..., U], dw f32 [..., U] -> (fill u8, depth f32)."""
    U = hit.shape[-1]
    x = np.broadcast_to(np.arange(U, dtype=np.int64), hit.shape)
    L = np.maximum.accumulate(np.where(hit, x, -1), axis=-1)                      # the last hit at or before
    R = np.minimum.accumulate(np.where(hit, x, U)[..., ::-1], axis=-1)[..., ::-1]  # the first hit at or after
    has_l, has_r = L >= 0, R < U
    dl = np.take_along_axis(dw, np.clip(L, 0, U - 1), axis=-1)
    dr = np.take_along_axis(dw, np.clip(R, 0, U - 1), axis=-1)
    n = R - L - 1
    hole = (~has_l & ~has_r) | ((max_gap > 0) & (n > max_gap))
    right = ~has_l | (has_l & has_r & (_z(dr, nearer) < _z(dl, nearer)))          # the farther bound; equal z: the left
    fill = np.where(hit, HIT, np.where(hole, HOLE, np.where(right, RIGHT, LEFT))).astype(np.uint8)
    depth = np.where(fill == HIT, dw, np.where(fill == LEFT, dl, np.where(fill == RIGHT, dr, F(0)))).astype(F)
    return fill, depth


def fill_loops(hit, dw, max_gap, nearer):
    """The same run by run: plain loops over the rows of [..., U]."""
    U = hit.shape[-1]
    fill, depth = np.zeros(hit.shape, np.uint8), np.zeros(hit.shape, F)
    h2, d2, f2, o2 = hit.reshape(-1, U), dw.reshape(-1, U), fill.reshape(-1, U), depth.reshape(-1, U)
    for r in range(h2.shape[0]):
        x = 0
        while x < U:
            if h2[r, x]:
                f2[r, x], o2[r, x] = HIT, d2[r, x]
                x += 1
                continue
            end = x
            while end < U and not h2[r, end]:
                end += 1
            has_l, has_r, n = x > 0, end < U, end - x
            if (has_l or has_r) and not (max_gap > 0 and n > max_gap):
                if has_l and has_r:
                    zl, zr = _z(d2[r, x - 1], nearer), _z(d2[r, end], nearer)
                    right = zr < zl
                else:
                    right = has_r
                f2[r, x:end] = RIGHT if right else LEFT
                o2[r, x:end] = d2[r, end] if right else d2[r, x - 1]
            x = end
    return fill, depth


def walk_order(S, t, exclude, radius):
    """The views by (distance to t, s), up to the first outside the radius, `exclude` left out -> [(s, distance f32)]."""
    dist = np.abs((np.arange(S).astype(F) - F(t)).astype(F))
    order = sorted(range(S), key=lambda s: (dist[s], s))
    return [(s, dist[s]) for s in order if (radius <= 0 or dist[s] <= F(radius)) and s != exclude]


def gather(depth, ok, slope, t, exclude, radius, sources, tol, fill, d, volume):
    """Stage C of one target: fill u8 / d f32 [V, U] -> n_src, colour (None without a volume), taken (a colour came from a view)."""
    S, V, U = depth.shape
    C = 0 if volume is None else volume.shape[3]
    x = np.broadcast_to(np.arange(U, dtype=np.int64), (V, U))
    vv = np.broadcast_to(np.arange(V, dtype=np.int64)[:, None], (V, U))
    nsrc, seen = np.zeros((V, U), np.int32), np.zeros((V, U), bool)
    wsum, acc, first = np.zeros((V, U), F), np.zeros((V, U, C), F), np.zeros((V, U, C), F)
    with np.errstate(all="ignore"):
        for s, dist in walk_order(S, t, exclude, radius):
            off = (d * F(F(s) - t)).astype(F)
            off = (off * slope).astype(F)
            near = np.abs(off) < F(1e9)                          # False for a NaN: nothing out of range is converted
            p = (x.astype(F) - np.where(near, off, F(0))).astype(F)
            ur = roundf(p)
            live = (fill != HOLE) & (nsrc < sources) & near & (ur >= 0) & (ur < U)
            urc = np.clip(ur, 0, U - 1)
            dt = depth[s][vv, urc]
            agrees = live & ok[s][vv, urc] & (np.abs((dt - d).astype(F)) <= tol)
            g = F(F(1) / F(F(1) + dist))
            if C:
                f0 = np.floor(p)
                w = (p - f0).astype(F)
                i0 = np.clip(f0.astype(np.int64), 0, U - 1)
                i1 = np.clip(np.ceil(p).astype(np.int64), 0, U - 1)
                e0, e1 = volume[vv, s, i0, :], volume[vv, s, i1, :]
                sample = (((F(1) - w).astype(F)[..., None] * e0).astype(F) + (w[..., None] * e1).astype(F)).astype(F)
                first = np.where((live & ~seen)[..., None], sample, first)
                acc = np.where(agrees[..., None], (acc + (g * sample).astype(F)).astype(F), acc)
            seen = seen | live
            wsum = np.where(agrees, (wsum + g).astype(F), wsum)
            nsrc = nsrc + agrees
            if not ((fill != HOLE) & (nsrc < sources)).any():
                break
        colour = np.where((nsrc > 0)[..., None], (acc / wsum[..., None]).astype(F), first).astype(F) if C else None
    return nsrc.astype(np.int32), colour, seen | (nsrc > 0)


def novel(depth, valid, slope, targets, exclude=None, radius=0, nearer=1, max_gap=0, sources=4, tol=np.inf, volume=None, want_err=False,
          fill_form=fill_vectorised):
    """-> dict of the planes: depth f32, fill u8, n_src i32 [T, V, U], row_cov i32 [T, V]; with a volume ([V, S, U, C] f32, as
    the slab holds it) colour f32 [T, V, U, C]; with want_err (every target a view) err f32 [T, V, U] and row_err f64 [T, V]."""
    assert sources >= 1 and tol >= 0
    a = wr.warp(depth, valid, slope, targets, exclude, radius, nearer)
    depth, ok, slope, targets, exclude = wr._args(depth, valid, slope, targets, exclude, nearer)
    tol = F(tol)
    T, (S, V, U) = len(targets), depth.shape
    fill, d = fill_form(a["hit"] != 0, a["depth"], max_gap, nearer)
    out = dict(depth=d, fill=fill, n_src=np.zeros((T, V, U), np.int32), row_cov=np.zeros((T, V), np.int32))
    if volume is not None:
        out["colour"] = np.zeros((T, V, U, volume.shape[3]), F)
    if want_err:
        out["err"], out["row_err"] = np.zeros((T, V, U), F), np.zeros((T, V), np.float64)
    for k, (t, ex) in enumerate(zip(targets, exclude)):
        nsrc, colour, taken = gather(depth, ok, slope, t, ex, radius, sources, tol, fill[k], d[k], volume)
        out["n_src"][k] = nsrc
        out["row_cov"][k] = (nsrc > 0).sum(axis=1)
        if volume is not None:
            out["colour"][k] = colour
        if want_err:
            L = volume[:, int(t), :, :]                              # [V, U, C]
            acc = np.zeros((V, U), F)
            for c in range(volume.shape[3]):                        # ascending, each addition rounded to binary32
                acc = (acc + np.abs((colour[..., c] - L[..., c]).astype(F))).astype(F)
            e = np.where(taken, (acc / F(volume.shape[3])).astype(F), F(0)).astype(F)
            out["err"][k] = e
            out["row_err"][k] = np.where(nsrc > 0, e, F(0)).astype(np.float64).sum(axis=1)
    return out


def hole_field(S, V, U, seed=0):
    """-> (depth, valid): view_warp_ref.tie_field with Gaussian jitter of 0.02, 5 % of the pixels invalid, and a band of 14
    invalid columns from 3 U / 4 in every view: cracks, disocclusions at the strip's sides and a gap no view fills."""
    rng = np.random.RandomState(77 + seed)
    depth = (wr.tie_field(S, V, U) + rng.normal(0.0, 0.02, (S, V, U)).astype(F)).astype(F)
    valid = np.where(rng.uniform(size=(S, V, U)) < 0.05, 0, 255).astype(np.uint8)
    valid[:, :, 3 * U // 4:3 * U // 4 + 14] = 0
    return depth, valid


@functools.lru_cache(maxsize=None)
def field(kind, S, V, U):
    """A field by name, computed once and shared (read-only): "hole" or "planted"."""
    depth, valid = hole_field(S, V, U) if kind == "hole" else planted(S, V, U)
    depth.setflags(write=False)
    valid.setflags(write=False)
    return depth, valid


@functools.lru_cache(maxsize=None)
def field_novel(kind, S, V, U, targets, exclude, radius, nearer=1, max_gap=0, sources=4, tol=0.1, slope=1.0, masked=True):
    """The yardstick on a named field, computed once and shared (read-only).  targets / exclude: tuples."""
    depth, valid = field(kind, S, V, U)
    out = novel(depth, valid if masked else None, slope, targets, exclude, radius, nearer, max_gap, sources, tol)
    for a in out.values():
        a.setflags(write=False)
    return out


def assert_equal(got, want, label, names=None):
    """Every plane bit for bit; row_err at 1e-9 relative (a double sum of at most 8192 binary32 values in any order)."""
    for k in (names if names is not None else [n for n in NAMES if n in want]):
        assert k in got, (label, k, "missing")
        if k == "row_err":
            assert got[k].shape == want[k].shape and got[k].dtype == np.float64, (label, k, got[k].shape, got[k].dtype)
            assert np.all(np.abs(got[k] - want[k]) <= 1e-9 * np.abs(want[k])), (label, k, np.abs(got[k] - want[k]).max())
            continue
        g, w = bits(got[k]), bits(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (label, k, g.shape, g.dtype, w.shape, w.dtype)
        bad = g != w
        assert not bad.any(), "%s: %s differs at %d pixels, first %s: got %r want %r" % (
            label, k, int(bad.sum()), tuple(np.argwhere(bad)[0]), got[k][tuple(np.argwhere(bad)[0])], want[k][tuple(np.argwhere(bad)[0])])
