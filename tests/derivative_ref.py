"""The rule of the derivative channels (K17; csrc/k17_derivative_rule.hpp, include/rslf_hip.h "derivative channels") in numpy,
float32 operation by operation: the yardstick of tests/test_derivative_cpu.py and tests/test_gpu_derivative.py.

    h  = float32(0.5) * float32(weight)
    fu = cap(|x[v][s][min(u+1, U-1)] - x[v][s][max(u-1, 0)]| * h, hi)
    fv = cap(|x[min(v+1, V-1)][s][u] - x[max(v-1, 0)][s][u]| * h, hi)         cap(f, hi) = hi where f > hi, else f

Float elements: hi = max(m, 0) with m the source's maximum.  Integer elements (uint8 / uint16 levels held as float32): the
product is rounded to the nearest integer, ties to even (np.rint), and hi is 255 / 65535."""
import numpy as np

F = np.float32
ELEMS = ("f32", "u8", "u16")
INT_HI = {"u8": F(255.0), "u16": F(65535.0)}


def pitch(U: int) -> int:
    """Pixels of a slab row (plan::volume_pitch): beyond U, a multiple of 64."""
    return (U + 1 + 63) // 64 * 64


def cap_of(x: np.ndarray, elem: str = "f32", m=None) -> np.float32:
    """hi of a source: the type's for integer elements, else max(m, 0) with m the source's maximum (default: x's)."""
    if elem != "f32":
        return INT_HI[elem]
    m = F(np.max(x)) if m is None else F(m)
    return m if m > 0 else F(0.0)


def _feature(after: np.ndarray, before: np.ndarray, h: np.float32, hi: np.float32, integer: bool) -> np.ndarray:
    d = (after - before).astype(F)
    f = (np.abs(d) * h).astype(F)
    if integer:
        f = np.rint(f).astype(F)
    return np.where(f > hi, hi, f).astype(F)


def augment(x_vsu: np.ndarray, weight: float, elem: str = "f32", hi=None) -> np.ndarray:
    """x [V, S, U] (or [V, S, U, 1]) float32 -> [V, S, U, 3] float32: (x, fu, fv)."""
    x = np.asarray(x_vsu, F)
    if x.ndim == 4:
        assert x.shape[3] == 1
        x = x[..., 0]
    V, S, U = x.shape
    h = F(0.5) * F(weight)
    hi = cap_of(x, elem) if hi is None else F(hi)
    integer = elem != "f32"
    u, v = np.arange(U), np.arange(V)
    fu = _feature(x[:, :, np.minimum(u + 1, U - 1)], x[:, :, np.maximum(u - 1, 0)], h, hi, integer)
    fv = _feature(x[np.minimum(v + 1, V - 1)], x[np.maximum(v - 1, 0)], h, hi, integer)
    return np.stack([x, fu, fv], axis=-1).astype(F)


def slab(x_vsu: np.ndarray, weight: float) -> np.ndarray:
    """The augmented volume as rslf_volume_describe shows it: [V][S][pitch][3] with a zero pad."""
    a = augment(x_vsu, weight)
    V, S, U, _ = a.shape
    out = np.zeros((V, S, pitch(U), 3), F)
    out[:, :, :U] = a
    return out


def augment_epis(epis, weight: float) -> list:
    """A list of V one-channel EPIs [S, U] (float32, uint8 or uint16) -> the list of V three-channel EPIs [S, U, 3] of the
    same dtype: what a pyramid with derivative_channels = weight runs on.  The integer features are integers within the
    type by the rule, so the cast back is exact."""
    a = np.stack([np.asarray(e) for e in epis])
    dt = a.dtype
    elem = {np.dtype(np.float32): "f32", np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16"}[np.dtype(dt)]
    out = augment(a.astype(F), weight, elem)
    if elem != "f32":
        assert (out == np.rint(out)).all() and out.min() >= 0 and out.max() <= INT_HI[elem]
    return [np.ascontiguousarray(out[v].astype(dt)) for v in range(out.shape[0])]
