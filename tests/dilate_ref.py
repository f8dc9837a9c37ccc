"""The dilation along u (K16, csrc/k16_dilate_rule.hpp) restated in numpy float32, op for op: the yardstick of
rslf_volume_dilate_u and of the stand-alone C++ program.  Also the band-limited small-slope field the feature is for.

A row of U columns becomes U' = f * (U - 1) + 1; column i * f + p lies at source coordinate i + p / f.  Phase 0 copies.
Every other phase: acc = w[0] * x[clamp(i - R + 1)], then acc = acc + w[m] * x[clamp(i - R + 1 + m)] for ascending m, each
product and each sum rounded to float32; out = min(max(acc, lo), hi) with lo, hi the source volume's min and max."""
import numpy as np

F = np.float32
LINEAR, CUBIC, LANCZOS3 = 0, 1, 2
KINDS = (LINEAR, CUBIC, LANCZOS3)
NAMES = {LINEAR: "linear", CUBIC: "cubic", LANCZOS3: "lanczos3"}


def radius(kind: int) -> int:
    return kind + 1


def dilated_width(U: int, f: int) -> int:
    return f * (U - 1) + 1


def pitch(U: int) -> int:
    """rslf_volume_create's rule: a multiple of 64, greater than U."""
    return (U + 1 + 63) // 64 * 64


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    px = 3.14159265358979323846 * x
    return float(np.sin(px)) / px


def kernel(kind: int, x: float) -> float:
    """h(x) in double."""
    a = abs(x)
    if kind == LINEAR:
        return 1.0 - a if a < 1.0 else 0.0
    if kind == CUBIC:   # Keys, a = -0.5
        if a <= 1.0:
            return (1.5 * a - 2.5) * a * a + 1.0
        if a < 2.0:
            return ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0
        return 0.0
    return _sinc(x) * _sinc(x / 3.0) if a < 3.0 else 0.0


def weights(kind: int, f: int) -> np.ndarray:
    """[f][T] float32: h in double, divided by the double sum (ascending), rounded to float."""
    R = radius(kind)
    T = 2 * R
    w = np.zeros((f, T), F)
    for p in range(f):
        d = [kernel(kind, p / f - (m - R + 1)) for m in range(T)]
        s = 0.0
        for x in d:
            s += x
        w[p] = [F(x / s) for x in d]
    w[0] = 0
    w[0, R - 1] = 1       # phase 0 is the column itself (never read: a copy)
    return w


def dilate(vol: np.ndarray, f: int, kind: int, lo=None, hi=None, clamp: bool = True) -> np.ndarray:
    """vol [..., U, C] float32 -> [..., U', C].  lo / hi: the source volume's min and max (default: of vol).  clamp=False:
    the sums as they are (what the range clamp acts on)."""
    vol = np.asarray(vol, F)
    U = vol.shape[-2]
    lo = F(vol.min()) if lo is None else F(lo)
    hi = F(vol.max()) if hi is None else F(hi)
    R = radius(kind)
    T = 2 * R
    w = weights(kind, f)
    out = np.zeros(vol.shape[:-2] + (dilated_width(U, f), vol.shape[-1]), F)
    out[..., ::f, :] = vol
    i = np.arange(U - 1)                       # the phases 1 .. f - 1 follow the columns 0 .. U - 2
    for p in range(1, f):
        acc = None
        for m in range(T):
            idx = np.clip(i - R + 1 + m, 0, U - 1)
            prod = (w[p, m] * vol[..., idx, :]).astype(F)
            acc = prod if acc is None else (acc + prod).astype(F)
        out[..., p::f, :] = np.fmin(np.fmax(acc, lo), hi) if clamp else acc
    return out


def slab(vol_vsuc: np.ndarray, f: int, kind: int) -> np.ndarray:
    """The dilated volume as rslf_volume_describe shows it: [V][S][pitch'][C] with a zero pad."""
    d = dilate(vol_vsuc, f, kind)
    V, S, Ud, C = d.shape
    out = np.zeros((V, S, pitch(Ud), C), F)
    out[:, :, :Ud] = d
    return out


# ---- the field of the issue: band-limited scanlines at small slopes ----------------------------------------------

def texture(rng, n=24, fmax=0.40):
    f = rng.uniform(0.02, fmax, n); a = rng.uniform(0.2, 1.0, n) / np.sqrt(n) * 0.6; ph = rng.uniform(0, 2*np.pi, n)
    return lambda x: 0.5 + 0.35 * np.sum(a[:, None] * np.sin(2*np.pi*f[:, None]*x[None, :] + ph[:, None]), 0) / 0.36


FIELD_V, FIELD_S, FIELD_U = 12, 9, 96
FIELD_D, FIELD_DMIN, FIELD_DMAX = 241, -0.6, 0.6
FIELD_MARGIN = 12


def small_slope_field(seed: int, V: int = FIELD_V, S: int = FIELD_S, U: int = FIELD_U):
    """(vol [V,S,U,1] float32 in [0, 1], delta [V]): view s of scanline v is clip(T(arange(U) - (S//2 - s) * delta[v]), 0, 1),
    one texture T per scanline, sampled exactly; delta = linspace(-0.45, 0.45, V)."""
    rng = np.random.default_rng(seed)
    delta = np.linspace(-0.45, 0.45, V)
    vol = np.zeros((V, S, U, 1), F)
    x = np.arange(U, dtype=np.float64)
    for v in range(V):
        T = texture(rng)
        for s in range(S):
            vol[v, s, :, 0] = np.clip(T(x - (S // 2 - s) * delta[v]), 0.0, 1.0).astype(F)
    return vol, delta


def field_mae(depth_raw: np.ndarray, edge_mask: np.ndarray, delta: np.ndarray, f: int = 1, U: int = FIELD_U) -> float:
    """Mean absolute error of depth_raw against the truth over the confident pixels of columns 12 .. U - 13 (of a dilated
    run only the columns f * u are read)."""
    d, m = depth_raw[:, ::f], edge_mask[:, ::f] != 0
    assert d.shape[1] == U
    sel = np.zeros_like(m)
    sel[:, FIELD_MARGIN:U - FIELD_MARGIN] = True
    sel &= m
    err = np.abs(d.astype(np.float64) - delta[:, None])
    return float(err[sel].mean())
