"""The yardstick of the cross-view consistency check (rslf_view_consistency): numpy, written from the rule as
include/rslf_hip.h states it, not from the kernel -- one view after the other over whole planes, every float operation a
single binary32 one in the order the rule gives.  Also the planted fields every test of the step runs on, and the conditions
that make them working ones."""
import functools

import numpy as np

F = np.float32
NAMES = ("seen", "agree", "above", "below", "fused", "valid")
TOL = 0.125
# (S, V, U, radius): U below a wave / above 256 and no multiple of it; S = 1; S = 9 and 17 (a batch of eight and a remainder);
# V = 1; a radius inside the view range and one that the range's edges cut
SHAPES = [(9, 3, 300, 0), (17, 2, 37, 0), (17, 2, 300, 4), (5, 1, 513, 2), (1, 2, 70, 0)]


def roundf(x):
    """C's roundf on float32 values below 2 ** 31 in magnitude: halves away from zero (in double, where |x| + 0.5 is exact)."""
    x = x.astype(np.float64)
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def ok_mask(depth, valid):
    ok = np.isfinite(depth)
    return ok if valid is None else ok & (valid != 0)


def consistency(depth, valid, slope, tol, radius=0, min_agree=0):
    """-> dict of the six planes [S, V, U]: seen / agree / above / below int32, fused float32, valid uint8."""
    depth = np.ascontiguousarray(depth, F)
    S, V, U = depth.shape
    slope, tol = F(slope), F(tol)
    ok = ok_mask(depth, valid)
    seen, agree, above, below = (np.zeros((S, V, U), np.int32) for _ in range(4))
    total = depth.copy()
    u = np.arange(U, dtype=np.int64)[None, :]
    with np.errstate(all="ignore"):
        for s in range(S):
            d = depth[s]
            for t in range(S):                                     # ascending: the order of the additions into `total`
                if t == s or (radius > 0 and abs(t - s) > radius):
                    continue
                off = (d * F(s - t)).astype(F)                      # two products, each rounded to binary32
                off = (off * slope).astype(F)
                near = np.abs(off) < F(1e9)                         # False for a NaN: nothing out of range is converted
                x = u + roundf(np.where(near, off, F(0)))
                in_field = ok[s] & near & (x >= 0) & (x < U)
                xc = np.clip(x, 0, U - 1)
                dt = np.take_along_axis(depth[t], xc, axis=1)
                there = in_field & np.take_along_axis(ok[t], xc, axis=1)
                diff = (dt - d).astype(F)
                ag = there & (np.abs(diff) <= tol)
                ab = there & ~ag & (diff > tol)
                be = there & ~ag & ~ab
                seen[s] += in_field
                agree[s] += ag
                above[s] += ab
                below[s] += be
                total[s] = np.where(ag, (total[s] + dt).astype(F), total[s])
        fused = np.where(ok, (total / (1 + agree).astype(F)).astype(F), F(0)).astype(F)
    out_valid = np.where(ok & (agree >= min_agree), 255, 0).astype(np.uint8)
    return dict(seen=seen, agree=agree, above=above, below=below, fused=fused, valid=out_valid)


@functools.lru_cache(maxsize=None)
def planted(S, V, U, seed=0, slope=1.0):
    """-> (depth [S, V, U] float32, valid [S, V, U] uint8), read-only: a background at disparity 0.5; a foreground strip at
    disparity 2.0, which the column rule moves from view to view (it hides the background); Gaussian jitter of 0.02; 15 % of
    the pixels replaced by uniform values in [-1, 3]; 10 % invalid; 1 % NaN."""
    rng = np.random.RandomState(1000 * seed + 7 * S + 3 * V + U)
    c = S // 2
    a, b = U // 3, U // 3 + max(4, U // 5)
    depth = np.full((S, V, U), 0.5, F)
    for s in range(S):
        shift = int(roundf(np.array([F(F(2.0) * F(c - s)) * F(slope)], F))[0])   # the strip's pixels of the centre view, in view s
        lo, hi = max(0, a + shift), min(U, b + shift)
        if lo < hi:
            depth[s, :, lo:hi] = 2.0
    depth += rng.normal(0.0, 0.02, depth.shape).astype(F)
    wild = rng.uniform(size=depth.shape) < 0.15
    depth[wild] = rng.uniform(-1.0, 3.0, int(wild.sum())).astype(F)
    valid = np.where(rng.uniform(size=depth.shape) < 0.10, 0, 255).astype(np.uint8)
    depth[rng.uniform(size=depth.shape) < 0.01] = np.nan
    depth.setflags(write=False)
    valid.setflags(write=False)
    return depth, valid


@functools.lru_cache(maxsize=None)
def planted_reference(S, V, U, radius, min_agree=0, seed=0, slope=1.0, tol=TOL, masked=True):
    """The yardstick on a planted field, computed once and shared (read-only)."""
    depth, valid = planted(S, V, U, seed, slope)
    out = consistency(depth, valid if masked else None, slope, tol, radius, min_agree)
    for a in out.values():
        a.setflags(write=False)
    return out


def shares(depth, valid, out):
    """The shares of the ok pixels that make a field a working one: agree > 0, above > 0, below > 0, seen below the field's
    maximum (some target out of field), fused != depth."""
    ok = ok_mask(depth, valid)
    n = max(1, int(ok.sum()))
    return dict(agree=float((out["agree"][ok] > 0).sum()) / n, above=float((out["above"][ok] > 0).sum()) / n,
                below=float((out["below"][ok] > 0).sum()) / n, partly_out=float((out["seen"][ok] < out["seen"].max()).sum()) / n,
                fused=float((out["fused"][ok].view(np.uint32) != np.ascontiguousarray(depth[ok], F).view(np.uint32)).sum()) / n)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def assert_equal_bitwise(got, want, label, names=NAMES):
    """Every plane, every pixel, fused included; NaNs cannot occur in an output, and would differ by their bits if they did."""
    for k in names:
        g, w = bits(got[k]), bits(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (label, k, g.shape, g.dtype, w.shape, w.dtype)
        bad = g != w
        assert not bad.any(), "%s: %s differs at %d pixels, first %s: got %r want %r" % (
            label, k, int(bad.sum()), tuple(np.argwhere(bad)[0]), got[k][tuple(np.argwhere(bad)[0])], want[k][tuple(np.argwhere(bad)[0])])
