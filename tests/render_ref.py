"""A numpy restatement of the reference's picture getters, written from the reference lines cited at each function
(paths relative to RSLightFields/).  It is the yardstick of tests/test_gpu_render.py and never imports the library.

Formulas run in np.float32, one operation at a time; cvRound is np.rint (nearest even); sorts are np.sort; the line
painter is the reference's loop, run sequentially.  Colour maps are tables: `lut` is a [256, 3] uint8 array and level i
becomes lut[i] (cv::applyColorMap is OpenCV's, not the reference's).

The readings of OpenCV this rests on (DESIGN.md section 5 lists them; none can be checked without OpenCV):
  * `Mat -= double` on CV_32F subtracts (float)min;
  * convertTo(CV_8U, a, b) from CV_32F computes x * (float)a + (float)b in float, unfused;
  * cvRound is nearest-even; a NaN, an infinity or a value beyond the int range converts to INT_MIN (cvtss2si), which
    saturate_cast<uchar> turns into 0 -- so a constant plane (max == min) renders lut[0] everywhere;
  * compare(Mat32F, double) compares against (float) of the scalar;
  * cv::meanStdDev: mean = sum * (1 / N), std = sqrt(max(sumsq * (1 / N) - mean * mean, 0)), sums in double.
"""
from __future__ import annotations

import math

import numpy as np

MINMAX, QUANTILE, MEANSTD = 0, 1, 2
SHIFT, AFFINE = 0, 1
BLACK, ZERO_VALUE = 0, 1
SQRT3 = 1.73205080757   # src/rslf_types.cpp:80-84


def cround(x: float) -> int:
    """(int)std::round(x) for a double: halves away from zero (Python's round is nearest-even)."""
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def centre_index(n: int) -> int:
    """(int)std::round(n / 2.0), include/rslf_fine_to_coarse.hpp:344, :497.  The reference then indexes with it; for
    n = 1 that is out of bounds, which is an error here."""
    i = cround(n / 2.0)
    if not 0 <= i < n:
        raise ValueError("round(%d / 2.0) = %d is out of range" % (n, i))
    return i


def scaled_row(v: int, dim_v: int, dim_v_orig: int) -> int:
    """(int)std::round(1.0 * v * dim_v / m_dim_v_orig_), include/rslf_fine_to_coarse.hpp:451; out of bounds is an error."""
    if not 0 <= v < dim_v_orig:
        raise ValueError("scanline %d of %d" % (v, dim_v_orig))
    i = cround(1.0 * v * dim_v / dim_v_orig)
    if not 0 <= i < dim_v:
        raise ValueError("row %d of %d" % (i, dim_v))
    return i


def zeroed(img: np.ndarray, valid) -> np.ndarray:
    """tmp.row(s).setTo(0.0, masks[s].row(v) == 0), include/rslf_fine_to_coarse.hpp:458-459"""
    img = np.asarray(img, np.float32)
    return img if valid is None else np.where(np.asarray(valid) != 0, img, np.float32(0.0)).astype(np.float32)


def fit(img: np.ndarray, mode: int, valid=None) -> tuple[float, float]:
    """The (min, max) doubles of copy_and_scale_uchar (src/rslf_plot.cpp:52-53: MINMAX) and of
    ImageConverter_uchar::fit (:65-98: QUANTILE for saturate, MEANSTD otherwise)."""
    x = zeroed(img, valid).reshape(-1)
    n = x.size
    if mode == MINMAX:
        return float(x.min()), float(x.max())
    if mode == QUANTILE:
        s = np.sort(x)                                   # cv::sort(..., CV_SORT_EVERY_COLUMN + CV_SORT_ASCENDING), :73
        return float(s[int(math.floor(0.02 * n))]), float(s[int(math.floor(0.98 * n))])   # :76-80
    d = x.astype(np.float64)
    total, total_sq = float(d.sum()), float((d * d).sum())
    scale = 1.0 / n
    mean = total * scale
    std = math.sqrt(max(total_sq * scale - mean * mean, 0.0))
    return float(x.min()), min(mean + 12 * std, float(x.max()))   # :92-94


def to_uchar(y: np.ndarray) -> np.ndarray:
    """cvRound + saturate_cast<uchar> of float levels."""
    with np.errstate(invalid="ignore"):
        r = np.rint(np.asarray(y, np.float32))
        in_int = np.abs(r) < np.float32(2147483648.0)     # false for NaN and the infinities
        return np.where(in_int, np.clip(r, 0, 255), 0).astype(np.uint8)


def levels(img: np.ndarray, vmin: float, vmax: float, formula: int) -> np.ndarray:
    """SHIFT: copy_and_scale_uchar, src/rslf_plot.cpp:54-56.  AFFINE: ImageConverter_uchar::copy_and_scale, :100-107."""
    x = np.asarray(img, np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        alpha = np.float32(np.float64(255.0) / (np.float64(vmax) - np.float64(vmin)))
        if formula == SHIFT:
            return to_uchar((x - np.float32(vmin)) * alpha)
        beta = np.float32(-np.float64(alpha) * np.float64(vmin))
        return to_uchar(x * alpha + beta)


def norms(radiance: np.ndarray) -> np.ndarray:
    """norm<float> / norm<cv::Vec3f> (src/rslf_types.cpp:80-91) over the last axis of [..., C]."""
    r = np.asarray(radiance, np.float32).astype(np.float64)
    if r.shape[-1] == 1:
        return (np.abs(r[..., 0]) * SQRT3).astype(np.float32)
    acc = r[..., 0] * r[..., 0]
    acc = acc + r[..., 1] * r[..., 1]
    acc = acc + r[..., 2] * r[..., 2]
    return np.sqrt(acc).astype(np.float32)


def render(img: np.ndarray, vmin: float, vmax: float, formula: int, lut: np.ndarray, valid=None, mask_mode: int = BLACK,
           radiance=None, shadow_level: float = 0.0) -> np.ndarray:
    """One plane [rows, cols] -> [rows, cols, 3]: level, table, mask, shadow cut (radiance: [rows, cols, C], normalised)."""
    x = zeroed(img, valid) if (valid is not None and mask_mode == ZERO_VALUE) else np.asarray(img, np.float32)
    out = np.asarray(lut, np.uint8)[levels(x, vmin, vmax, formula)]
    if valid is not None and mask_mode == BLACK:
        out[np.asarray(valid) == 0] = 0
    if radiance is not None:
        out[norms(radiance) < np.float32(shadow_level)] = 0
    return out


def epi_lines(depth_u: np.ndarray, mask_u: np.ndarray, S: int, s_hat: int, lut: np.ndarray, lowest_column: int = 0) -> np.ndarray:
    """Depth1DComputer_pile::get_coloured_epi, include/rslf_depth_computation.hpp:580-617, its loop run sequentially
    (lowest_column = 0: `requested_index > -1`); Depth1DComputer::get_coloured_epi, :385-413, with lowest_column = 1
    (`requested_index > 0`)."""
    depth_u = np.asarray(depth_u, np.float32)
    U = depth_u.size
    occlusion = np.full((S, U), -np.inf, np.float32)
    colours = np.asarray(lut, np.uint8)[levels(depth_u, float(depth_u.min()), float(depth_u.max()), SHIFT)]
    out = np.zeros((S, U, 3), np.uint8)
    for u in range(U):
        if not mask_u[u]:
            continue
        d = depth_u[u]
        for s in range(S):
            p = float(np.float32(d) * np.float32(s_hat - s))
            if not abs(p) < 1e9:   # NaN or beyond every row: the reference's conversion to int is undefined
                continue
            t = u + cround(p)
            if lowest_column <= t < U and occlusion[s, t] < d:
                out[s, t] = colours[u]
                occlusion[s, t] = d
    return out


# ---- the getters ------------------------------------------------------------------------------------------------------

def pile_coloured_epi(depth_vu, mask_vu, S, s_hat, lut, a_v=-1):
    """include/rslf_depth_computation.hpp:568-617"""
    V = depth_vu.shape[0]
    if a_v < 0:
        a_v = int(math.floor(V / 2.0))
    return epi_lines(depth_vu[a_v], mask_vu[a_v], S, s_hat, lut)


def disparity_map(depth_vu, mask_vu, lut):
    """Depth1DComputer_pile::get_disparity_map, :619-643, and Depth2DComputer::get_disparity_map for its plane, :858-891"""
    vmin, vmax = fit(depth_vu, MINMAX)
    return render(depth_vu, vmin, vmax, SHIFT, lut, mask_vu, BLACK)


def depth2d_coloured_epi(depth_svu, mask_svu, lut, a_v=-1):
    """include/rslf_depth_computation.hpp:808-856"""
    V = depth_svu.shape[1]
    if a_v < 0:
        a_v = int(math.floor(V / 2.0))
    return disparity_map(np.ascontiguousarray(depth_svu[:, a_v, :]), mask_svu[:, a_v, :], lut)


def f2c_coloured_depth_maps(out_map_svu, out_valid_svu, lut, saturate=True, radiance_vsuc=None, shadow_level=0.0):
    """include/rslf_fine_to_coarse.hpp:325-378; radiance_vsuc: level 0's normalised EPIs [V, S, U, C] with par_cut_shadows"""
    S = out_map_svu.shape[0]
    vmin, vmax = fit(out_map_svu[centre_index(S)], QUANTILE if saturate else MEANSTD)
    return np.stack([render(out_map_svu[s], vmin, vmax, AFFINE, lut, out_valid_svu[s], BLACK,
                            None if radiance_vsuc is None else radiance_vsuc[:, s], shadow_level) for s in range(S)])


def f2c_coloured_depth_pyr(depths, valids, lut, s=-1, saturate=True):
    """include/rslf_fine_to_coarse.hpp:491-519; depths / valids: per level [S, V_p, U_p]"""
    if s == -1:
        s = centre_index(depths[0].shape[0])
    vmin, vmax = fit(depths[0][s], QUANTILE if saturate else MEANSTD)
    return [render(d[s], vmin, vmax, AFFINE, lut, m[s], BLACK) for d, m in zip(depths, valids)]


def f2c_coloured_epi_pyr(depths, valids, lut, v=-1, saturate=True, radiances=None, shadow_level=0.0):
    """include/rslf_fine_to_coarse.hpp:432-488; radiances: per level the normalised EPIs [V_p, S, U_p, C] with par_cut_shadows"""
    V0 = depths[0].shape[1]
    if v == -1:
        v = centre_index(V0)
    out, vmin, vmax = [], 0.0, 0.0
    for p, (d, m) in enumerate(zip(depths, valids)):
        row = scaled_row(v, d.shape[1], V0)
        plane, mask = np.ascontiguousarray(d[:, row, :]), m[:, row, :]
        if p == 0:
            vmin, vmax = fit(plane, QUANTILE if saturate else MEANSTD, mask)
        out.append(render(plane, vmin, vmax, AFFINE, lut, mask, ZERO_VALUE, None if radiances is None else radiances[p][row], shadow_level))
    return out
