"""The rule of the per-view equalisation (K19; csrc/k19_equalize_rule.hpp, include/rslf_hip.h "per-view equalisation") in
numpy, its three parts apart: the statistics in numpy integers, the coefficients in float64, the apply pass in float32,
operation by operation.  The yardstick of tests/test_equalize_cpu.py and tests/test_gpu_equalize.py.

    k = float32(65535) / hi                                                     one binary32 division
    q(x) = uint32(min(rint(min(max(x, 0), hi) * k), 65535))                     a NaN is not counted
    n, s1, s2 = #counted, sum q, sum q^2  per view s and channel c over all (v, u)             uint64
    m = s1 / n / 65535 * hi,  sd = sqrt(max(s2 / n / 65535^2 * hi^2 - m^2, 0))                 float64
    GAIN: a = mt / m (m > 0), b = 0;  AFFINE: a = sdt / sd (sd > 0), b = mt - a m;  a clamped to [1 / max_gain, max_gain]
    y = x * a + b (float32 multiply, then add), integer elements rint, then clamped to [0, hi]; NaN and (1, 0) copy x"""
import numpy as np

F = np.float32
ELEMS = ("f32", "u8", "u16")
INT_HI = {"u8": F(255.0), "u16": F(65535.0)}
GAIN, AFFINE = 1, 2


def pitch(U: int) -> int:
    """Pixels of a slab row (plan::volume_pitch): beyond U, a multiple of 64."""
    return (U + 1 + 63) // 64 * 64


def cap_of(x: np.ndarray, elem: str = "f32") -> np.float32:
    """hi of a field: the type's for integer elements, else its maximum (NaNs apart)."""
    return INT_HI[elem] if elem != "f32" else F(np.nanmax(x))


def _vsuc(x):
    x = np.asarray(x, F)
    return x[..., None] if x.ndim == 3 else x


def view_stats(x_vsuc: np.ndarray, hi) -> np.ndarray:
    """x [V, S, U(, C)] float32 -> uint64 [S, C, 3]: (n, s1, s2) per view and channel."""
    x = _vsuc(x_vsuc)
    hi = F(hi)
    k = F(F(65535.0) / hi)
    counted = ~np.isnan(x)
    with np.errstate(invalid="ignore"):
        c = np.minimum(np.maximum(x, F(0.0)), hi).astype(F)
        p = (c * k).astype(F)
        r = np.minimum(np.rint(p), F(65535.0)).astype(F)
    q = np.where(counted, r, F(0.0)).astype(np.uint64)
    out = np.zeros((x.shape[1], x.shape[3], 3), np.uint64)
    out[..., 0] = counted.sum(axis=(0, 2), dtype=np.uint64)
    out[..., 1] = q.sum(axis=(0, 2), dtype=np.uint64)
    out[..., 2] = (q * q).sum(axis=(0, 2), dtype=np.uint64)
    return out


def _moments(t, hi):
    """(n, s1, s2) uint64 -> (m, sd, counted) in float64."""
    n, s1, s2 = (np.uint64(v) for v in t)
    if n == 0:
        return 0.0, 0.0, False
    dn, h = np.float64(n), np.float64(hi)
    m = np.float64(s1) / dn / np.float64(65535.0) * h
    e2 = np.float64(s2) / dn / (np.float64(65535.0) * np.float64(65535.0)) * (h * h)
    var = e2 - m * m
    return m, np.sqrt(var if var > 0.0 else np.float64(0.0)), True


def coefficients(stats: np.ndarray, hi, mode: int, ref_view: int, joint: bool, max_gain: float = 4.0) -> np.ndarray:
    """stats uint64 [S, C, 3] -> float32 [S, C, 2] (a, b).  ref_view -1: the mean of the views with n > 0."""
    stats = np.asarray(stats, np.uint64)
    S, C_ = stats.shape[:2]
    assert mode in (GAIN, AFFINE) and -1 <= ref_view < S and (not joint or C_ == 3)
    hi = F(hi)
    gmax = np.float64(F(max_gain))
    gmin = np.float64(1.0) / gmax
    out = np.zeros((S, C_, 2), F)
    groups = [list(range(C_))] if joint else [[c] for c in range(C_)]
    for chans in groups:
        tot = stats[:, chans, :].sum(axis=1, dtype=np.uint64)          # [S, 3]: the channels' integers added first
        mom = [_moments(tot[s], hi) for s in range(S)]
        if ref_view >= 0:
            mt, sdt, target = mom[ref_view]
        else:
            seen = [(m, sd) for m, sd, ok in mom if ok]
            target = len(seen) > 0
            mt = sdt = np.float64(0.0)
            if target:
                sm = ssd = np.float64(0.0)
                for m, sd in seen:                                        # in view order
                    sm, ssd = sm + m, ssd + sd
                mt, sdt = sm / np.float64(len(seen)), ssd / np.float64(len(seen))
        for s in range(S):
            m, sd, ok = mom[s]
            a, b = np.float64(1.0), np.float64(0.0)
            if target and ok and s != ref_view:
                if mode == GAIN:
                    a = mt / m if m > 0.0 else np.float64(1.0)
                else:
                    a = sdt / sd if sd > 0.0 else np.float64(1.0)
                a = gmin if a < gmin else (gmax if a > gmax else a)
                if mode == AFFINE:
                    b = mt - a * m
            out[s, chans, 0] = F(a)
            out[s, chans, 1] = F(b)
    return out


def apply(x_vsuc: np.ndarray, a_b: np.ndarray, hi, elem: str = "f32") -> np.ndarray:
    """y = a x + b per view and channel, the shape of x."""
    x4 = _vsuc(x_vsuc)
    a_b = np.asarray(a_b, F)
    hi = F(hi)
    a = a_b[None, :, None, :, 0]
    b = a_b[None, :, None, :, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        p = (x4 * a).astype(F)
        y = (p + b).astype(F)
        if elem != "f32":
            y = np.rint(y).astype(F)
        y = np.where(y < 0, F(0.0), np.where(y > hi, hi, y)).astype(F)
    copy = np.isnan(x4) | np.broadcast_to((a == 1) & (b == 0), x4.shape)
    y = np.where(copy, x4, y).astype(F)
    return y.reshape(np.asarray(x_vsuc).shape)


def equalize(x_vsuc: np.ndarray, mode: int = AFFINE, ref_view=None, joint=None, max_gain: float = 4.0, elem: str = "f32", hi=None):
    """The three parts in a row -> (y, a_b, stats).  ref_view None: the view S // 2; joint None: on for three channels."""
    x4 = _vsuc(x_vsuc)
    S, C_ = x4.shape[1], x4.shape[3]
    hi = cap_of(x4, elem) if hi is None else F(hi)
    ref = S // 2 if ref_view is None else ref_view
    j = (C_ == 3) if joint is None else bool(joint)
    st = view_stats(x4, hi)
    a_b = coefficients(st, hi, mode, ref, j, max_gain)
    return apply(x_vsuc, a_b, hi, elem), a_b, st


def slab(y_vsuc: np.ndarray) -> np.ndarray:
    """A field as rslf_volume_describe shows its volume: [V][S][pitch][C] with a zero pad."""
    y = _vsuc(y_vsuc)
    V, S, U, C_ = y.shape
    out = np.zeros((V, S, pitch(U), C_), F)
    out[:, :, :U] = y
    return out


def equalize_epis(epis, mode: int = AFFINE, ref_view=None, joint=None, max_gain: float = 4.0):
    """A list of V EPIs [S, U] / [S, U, 3] (float32, uint8 or uint16) -> (the list of V equalised EPIs of the same dtype, a_b):
    what a pyramid with equalize_views = mode runs on.  The integer results are integers within the type by the rule, so the
    cast back is exact."""
    a = np.stack([np.asarray(e) for e in epis])
    dt = a.dtype
    elem = {np.dtype(np.float32): "f32", np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16"}[np.dtype(dt)]
    y, a_b, _ = equalize(a.astype(F), mode, ref_view, joint, max_gain, elem)
    if elem != "f32":
        assert (y == np.rint(y)).all() and y.min() >= 0 and y.max() <= INT_HI[elem]
    return [np.ascontiguousarray(y[v].astype(dt)) for v in range(y.shape[0])], a_b
