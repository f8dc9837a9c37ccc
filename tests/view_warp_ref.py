"""The yardstick of the view warp (rslf_view_warp): numpy, written from the rule as include/rslf_hip.h states it, not from the
kernel -- no keys, no ranks, no walk: the candidates of a target row are sorted by (column, z descending, view distance, view)
and the first of each column wins.  A plain triple loop over (s, v, u), which keeps the best candidate per column by the same
three comparisons, checks the vectorised form on a small shape.  The planted fields are tests/consistency_ref.py's."""
import functools

import numpy as np

from consistency_ref import bits, ok_mask, planted, roundf

F = np.float32
NAMES = ("hit", "depth", "src_view", "src_col", "count", "colour", "err", "row_err", "row_hits")
PLANES = NAMES[:5]   # what a call without a volume can give (and row_hits)
DTYPES = dict(hit=np.uint8, depth=F, src_view=np.int32, src_col=np.int32, count=np.int32, colour=F, err=F, row_err=np.float64,
              row_hits=np.int32)


def _candidates(depth, ok, s, t, slope, exclude, radius):
    """-> (mask [V, U], x [V, U] int64) of view s for target t."""
    V, U = depth.shape[1:]
    dist = F(np.abs(F(F(s) - t)))
    if s == exclude or (radius > 0 and not dist <= F(radius)):
        return np.zeros((V, U), bool), np.zeros((V, U), np.int64)
    with np.errstate(all="ignore"):
        off = (depth[s] * F(F(s) - t)).astype(F)            # two products, each rounded to binary32
        off = (off * slope).astype(F)
        near = np.abs(off) < F(1e9)                         # False for a NaN: nothing out of range is converted
    x = np.arange(U, dtype=np.int64)[None, :] + roundf(np.where(near, off, F(0)))
    return ok[s] & near & (x >= 0) & (x < U), x


def _empty(T, V, U, C, want_err):
    out = dict(hit=np.zeros((T, V, U), np.uint8), depth=np.zeros((T, V, U), F), src_view=np.full((T, V, U), -1, np.int32),
               src_col=np.full((T, V, U), -1, np.int32), count=np.zeros((T, V, U), np.int32), row_hits=np.zeros((T, V), np.int32))
    if C:
        out["colour"] = np.zeros((T, V, U, C), F)
    if want_err:
        out["err"] = np.zeros((T, V, U), F)
        out["row_err"] = np.zeros((T, V), np.float64)
    return out


def _radiances(out, volume, targets, want_err):
    """colour, err, row_err and row_hits from the winners: volume [V, S, U, C] float32 as the slab holds it."""
    T, V, U = out["hit"].shape
    hit = out["hit"] != 0
    out["row_hits"][...] = hit.sum(axis=2)
    if volume is None:
        return out
    C = volume.shape[3]
    for k in range(T):
        for v in range(V):
            x = np.nonzero(hit[k, v])[0]
            col = volume[v, out["src_view"][k, v, x], out["src_col"][k, v, x], :]
            out["colour"][k, v, x, :] = col
            if want_err:
                L = volume[v, int(targets[k]), x, :]
                acc = np.zeros(len(x), F)
                for c in range(C):                              # ascending, each addition rounded to binary32
                    acc = (acc + np.abs((col[:, c] - L[:, c]).astype(F))).astype(F)
                e = (acc / F(C)).astype(F)
                out["err"][k, v, x] = e
                out["row_err"][k, v] = e.astype(np.float64).sum()
    return out


def _args(depth, valid, slope, targets, exclude, nearer):
    depth = np.ascontiguousarray(depth, F)
    targets = [F(t) for t in targets]
    exclude = [-1] * len(targets) if exclude is None else [int(e) for e in exclude]
    assert nearer != 0 and len(exclude) == len(targets)
    return depth, ok_mask(depth, valid), F(slope), targets, exclude


def warp(depth, valid, slope, targets, exclude=None, radius=0, nearer=1, volume=None, want_err=False):
    """-> dict of the planes: hit u8, depth f32, src_view / src_col / count i32 [T, V, U], row_hits i32 [T, V]; with a volume
    colour f32 [T, V, U, C]; with want_err (every target a view) err f32 [T, V, U] and row_err f64 [T, V]."""
    depth, ok, slope, targets, exclude = _args(depth, valid, slope, targets, exclude, nearer)
    S, V, U = depth.shape
    out = _empty(len(targets), V, U, 0 if volume is None else volume.shape[3], want_err)
    u_of = np.broadcast_to(np.arange(U, dtype=np.int64), (S, U))
    s_of = np.broadcast_to(np.arange(S, dtype=np.int64)[:, None], (S, U))
    for k, (t, ex) in enumerate(zip(targets, exclude)):
        cand = [_candidates(depth, ok, s, t, slope, ex, radius) for s in range(S)]
        mask, x = np.stack([c[0] for c in cand]), np.stack([c[1] for c in cand])   # [S, V, U]
        dist = np.abs((np.arange(S).astype(F) - t).astype(F))
        for v in range(V):
            m = mask[:, v, :]
            xs, ss, us = x[:, v, :][m], s_of[m], u_of[m]
            d = depth[:, v, :][m]
            z = (d if nearer >= 0 else -d) + F(0)              # -0.0 + 0.0 = +0.0: the two zeros are one depth
            order = np.lexsort((ss, dist[ss], -z, xs))          # column; then z descending, distance, view
            xs, ss, us, d = xs[order], ss[order], us[order], d[order]
            first = np.ones(len(xs), bool)
            first[1:] = xs[1:] != xs[:-1]
            w = xs[first]
            out["hit"][k, v, w] = 255
            out["depth"][k, v, w] = d[first]
            out["src_view"][k, v, w] = ss[first]
            out["src_col"][k, v, w] = us[first]
            out["count"][k, v] = np.bincount(xs, minlength=U)
    return _radiances(out, volume, targets, want_err)


def warp_loops(depth, valid, slope, targets, exclude=None, radius=0, nearer=1, volume=None, want_err=False):
    """The same by a plain triple loop over (s, v, u): the best candidate so far of a column is replaced when the new one has a
    greater z, or an equal z and a smaller distance, or both equal and a smaller s."""
    depth, ok, slope, targets, exclude = _args(depth, valid, slope, targets, exclude, nearer)
    S, V, U = depth.shape
    out = _empty(len(targets), V, U, 0 if volume is None else volume.shape[3], want_err)
    for k, (t, ex) in enumerate(zip(targets, exclude)):
        best = {}
        for s in range(S):
            mask, x = _candidates(depth, ok, s, t, slope, ex, radius)
            dist = F(np.abs(F(F(s) - t)))
            for v in range(V):
                for u in range(U):
                    if not mask[v, u]:
                        continue
                    d = depth[s, v, u]
                    z = d if nearer >= 0 else -d
                    cell = (v, int(x[v, u]))
                    out["count"][(k,) + cell] += 1
                    b = best.get(cell)
                    if b is None or z > b[0] or (z == b[0] and (dist < b[1] or (dist == b[1] and s < b[2]))):
                        best[cell] = (z, dist, s, u, d)
        for cell, (z, dist, s, u, d) in best.items():
            out["hit"][(k,) + cell] = 255
            out["depth"][(k,) + cell] = d
            out["src_view"][(k,) + cell] = s
            out["src_col"][(k,) + cell] = u
    return _radiances(out, volume, targets, want_err)


@functools.lru_cache(maxsize=None)
def planted_warp(S, V, U, radius, targets, exclude=None, nearer=1, slope=1.0, masked=True, seed=0):
    """The yardstick on a planted field (consistency_ref.planted), computed once and shared (read-only).  targets / exclude:
    tuples."""
    depth, valid = planted(S, V, U, seed, abs(slope))
    out = warp(depth, valid if masked else None, slope, targets, exclude, radius, nearer)
    for a in out.values():
        a.setflags(write=False)
    return out


def leave_one_out(S):
    """Every view as a target, each excluded from its own prediction -> (targets, exclude), tuples."""
    return tuple(float(s) for s in range(S)), tuple(range(S))


def tie_field(S=9, V=2, U=120):
    """The background 0.5 and the strip 2.0 of `planted` without jitter, outliers, invalids or NaN: whole regions of equal
    disparity, so that several views send the SAME z to a column and the distance-then-s order decides."""
    c = S // 2
    a, b = U // 3, U // 3 + max(4, U // 5)
    depth = np.full((S, V, U), 0.5, F)
    for s in range(S):
        shift = int(roundf(np.array([F(F(2.0) * F(c - s))], F))[0])
        lo, hi = max(0, a + shift), min(U, b + shift)
        if lo < hi:
            depth[s, :, lo:hi] = 2.0
    return depth


def tied_share(depth, valid, slope, t, exclude, radius=0, nearer=1):
    """Of the hit pixels of target t: the share whose runner-up has the winner's z (the second of a column's sorted candidates)."""
    depth, ok, slope, (t,), (ex,) = _args(depth, valid, slope, [t], [exclude], nearer)
    S, V, U = depth.shape
    tied = hits = 0
    for v in range(V):
        zs = [[] for _ in range(U)]
        for s in range(S):
            mask, x = _candidates(depth, ok, s, t, slope, ex, radius)
            for u in np.nonzero(mask[v])[0]:
                d = depth[s, v, u]
                zs[int(x[v, u])].append(float(d if nearer >= 0 else -d))
        for col in zs:
            if col:
                hits += 1
                col.sort(reverse=True)
                tied += len(col) > 1 and col[0] == col[1]
    return tied / max(1, hits)


def normalised(volume_u8):
    """A uint8 light field [V, S, U, C] as the slab holds it after K0: F(x) * F(1 / 255)."""
    return (volume_u8.astype(F) * F(1.0 / 255.0)).astype(F)


def assert_equal(got, want, label, names=None):
    """Every plane bit for bit; row_err at 1e-9 relative: a double sum of at most 16384 binary32 values in any order is within
    U * 2^-53, about 2e-12, of the exact one."""
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
