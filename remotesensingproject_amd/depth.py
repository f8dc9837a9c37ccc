"""Host-side mirror of the reference's interface for the 1-D pile path.

Names, argument meaning and defaults follow RSLightFields
(/root/reference/RSLightFields/include/):
  Depth1DParameters                 rslf_depth_computation_core.hpp:66-142
  compute_1D_edge_confidence_pile   rslf_depth_computation_core.hpp:279-287
  compute_1D_depth_epi_pile         rslf_depth_computation_core.hpp:293-310
  selective_median_filter           rslf_depth_computation_core.hpp:366-375
  Depth1DComputer_pile              rslf_depth_computation.hpp:93-143, :425-565
The reference's `Mat`s become torch CUDA tensors (device memory + streams are
all torch is used for); the arithmetic runs in librslf_hip.so through the C-ABI
of include/rslf_hip.h.  No CPU path exists here.
"""
from __future__ import annotations

import atexit
import copy
import ctypes as C
import sys
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import RslfParams, RslfStats, RslfVolumeDesc, check


class Interpolation1DLinear:
    """include/rslf_interpolation.hpp:59-67, :155-193 (RSLF_INTERP_LINEAR)."""
    mode = 0


class Interpolation1DNearestNeighbour:
    """include/rslf_interpolation.hpp:46-54.  `as_built=False`: the class as its scalar interpolate() states it
    (:80-92, RSLF_INTERP_NEAREST).  `as_built=True`: what interpolate_mat() executes in the reference, the float
    index matrix read through an int pointer (:118, RSLF_INTERP_NEAREST_AS_BUILT)."""

    def __init__(self, as_built: bool = False):
        self.mode = 2 if as_built else 1


@dataclass
class Depth1DParameters:
    """rslf::Depth1DParameters<T> with the reference's member names and defaults."""

    par_edge_score_threshold: float = 0.02
    par_line_score_threshold: float = 0.02
    par_disp_score_threshold: float = 0.01
    par_raw_score_threshold: float = 0.0
    par_mean_shift_max_iter: float = 10.0
    par_edge_confidence_filter_size: int = 9
    par_edge_confidence_opening_type: int = 2
    par_edge_confidence_opening_size: int = 1
    par_median_filter_size: int = 5
    par_median_filter_epsilon: float = 0.1
    par_propagation_epsilon: float = 0.1
    par_slope_factor: float = 1.0
    par_cut_shadows: bool = True
    par_shadow_level: float = 0.05 * 1.73205080757
    par_kernel_bandwidth: float = 0.2   # BandwidthKernel(_BANDWIDTH_KERNEL_PARAMETER), core.hpp:78
    # par_interpolation_class (core.hpp:76-77, :108): an Interpolation1DLinear / Interpolation1DNearestNeighbour
    # instance, or the RSLF_INTERP_* integer itself
    par_interpolation_class: object = 0
    # the reference's commented-out build switch _USE_DISP_CONFIDENCE_SCORE (core.hpp:35): propagation gated by
    # C_d > par_disp_score_threshold instead of the edge mask
    par_use_disp_confidence_score: bool = False
    # the reference's build switch _USE_LINE_CONFIDENCE_SCORE (core.hpp:1032-1081), a LINE_CONF_* mode of the 2-D sweep:
    # 0 off; 1 as built (C_l computed and carried, the gate stays the edge mask: the gating branches sit behind an
    # `#elseif` typo); 2 gate (propagation, getters and validity under C_l > par_line_score_threshold, what those branches
    # say).  Host-side only: it is an argument of the *_lc entry points, not a member of rslf_params.
    par_line_confidence_mode: int = 0

    @staticmethod
    def get_default() -> "Depth1DParameters":
        return Depth1DParameters()

    def to_c(self) -> RslfParams:
        p = RslfParams()
        for f, _ in RslfParams._fields_:
            if f == "interpolation":
                p.interpolation = int(getattr(self.par_interpolation_class, "mode", self.par_interpolation_class))
                continue
            v = getattr(self, "par_" + f)
            setattr(p, f, int(v) if isinstance(getattr(p, f), int) else float(v))
        return p


LINE_CONF_OFF, LINE_CONF_AS_BUILT, LINE_CONF_GATE = 0, 1, 2   # RSLF_LINE_CONF_*


def require_no_line_confidence(parameters, who: str) -> None:
    """The line confidence is built for the one-device Depth2DComputer alone (DESIGN.md 3 "K7"): every other path that
    takes parameters refuses a mode other than 0 instead of ignoring it or running it untested."""
    if parameters is not None and int(parameters.par_line_confidence_mode) != LINE_CONF_OFF:
        raise ValueError("%s: par_line_confidence_mode=%d is not built here (one-device Depth2DComputer only)"
                         % (who, int(parameters.par_line_confidence_mode)))


def require_no_subgrid(subgrid, who: str) -> None:
    """The sub-grid mode is built for one device -- the pile step (DESIGN.md 3 "Sub-grid pile"), the 2-D sweep and the
    pyramid ("Sub-grid sweep") -- and every multi-device form refuses it instead of ignoring it."""
    if subgrid:
        raise ValueError("%s: subgrid=True is not built here (one device: Depth1DComputer_pile, Depth1DComputer, "
                         "Depth2DComputer, FineToCoarse, fine_to_coarse_run_host and the compute_*_depth_epi functions)" % who)


def require_no_peaks(peaks, who: str) -> None:
    """The peaks mode of the 2-D sweep (DESIGN.md 3 "Sweep peaks") is built for Depth2DComputer and compute_2D_depth_epi on
    one device; the pyramid and every multi-device form refuse it instead of ignoring it."""
    if peaks is not None and peaks is not False:
        raise ValueError("%s: peaks is not built here (one device, one sweep: Depth2DComputer and compute_2D_depth_epi)" % who)


def _ratio_on(ratio) -> bool:
    return ratio is not None and ratio is not False and ratio != 0


def require_no_propagation_ratio(ratio, who: str) -> None:
    """The sweep gate (DESIGN.md 3 "Sweep gate") is built where the peaks mode is and for a kept pyramid: one device.  Every
    other form refuses it instead of ignoring it."""
    if _ratio_on(ratio):
        raise ValueError("%s: propagation_ratio is not built here (one device, a sweep in the peaks mode: Depth2DComputer, "
                         "compute_2D_depth_epi and fine_to_coarse_run_host(keep=True, peaks=True))" % who)


def require_no_consistency_gate(min_agree, who: str) -> None:
    """A pyramid's validity by cross-view consistency (DESIGN.md 3 "Consistency gate") is built for a kept run on one device.
    Every other form refuses it instead of ignoring it."""
    if min_agree is not None and min_agree is not False and min_agree != 0:
        raise ValueError("%s: consistency_min_agree is not built here (one device, a kept run: fine_to_coarse_run_host(keep=True))" % who)


def _propagation_ratio(ratio, who: str) -> float:
    """None / 0 -> 0.0 (off); else a ratio in (0, 1] (a NaN is none)."""
    if not _ratio_on(ratio):
        return 0.0
    r = float(ratio)
    if not 0.0 < r <= 1.0:
        raise ValueError("%s: propagation_ratio %r is not in (0, 1]" % (who, ratio))
    return r


DILATE_LINEAR, DILATE_CUBIC, DILATE_LANCZOS3 = 0, 1, 2   # RSLF_DILATE_*
DILATE_MAX_FACTOR = 8                                     # kDilateMaxFactor (csrc/k16_dilate_rule.hpp)


def _u_dilation(u_dilation, dilation_kind, who: str) -> tuple[int, int]:
    """(factor, kind) of the u_dilation / dilation_kind arguments; a factor is an integer in 1..8, a kind a DILATE_*."""
    f = 1 if u_dilation is None else u_dilation
    if isinstance(f, bool) or int(f) != f or not 1 <= int(f) <= DILATE_MAX_FACTOR:
        raise ValueError("%s: u_dilation %r is not an integer in 1..%d" % (who, u_dilation, DILATE_MAX_FACTOR))
    if dilation_kind not in (DILATE_LINEAR, DILATE_CUBIC, DILATE_LANCZOS3):
        raise ValueError("%s: dilation_kind %r is not DILATE_LINEAR, DILATE_CUBIC or DILATE_LANCZOS3" % (who, dilation_kind))
    return int(f), int(dilation_kind)


def require_no_u_dilation(u_dilation, who: str) -> None:
    """The dilation along u (DESIGN.md 3 "K16") is built for one device and one level: Depth1DComputer_pile, Depth1DComputer
    and Depth2DComputer.  The pyramid's levels are never dilated -- its form is the level dilation, which dilates each
    level's sweep alone (level_dilation=, DESIGN.md 3 "K18") -- and every multi-device or sharded form would have to dilate
    per chunk: they refuse it instead of ignoring it."""
    if u_dilation is not None and u_dilation != 1:
        raise ValueError("%s: u_dilation=%r is not built here (one device, one level: Depth1DComputer_pile, Depth1DComputer, "
                         "Depth2DComputer; or Volume.dilated_u and a slope factor of your own)" % (who, u_dilation))


def require_no_line_confidence_dilated(parameters, u_dilation: int, who: str) -> None:
    """K7 samples C_e along u + (s_hat - s) * d with no slope factor, as the reference writes it (core.hpp:1058): in a
    dilated frame it would walk the wrong line."""
    if u_dilation != 1 and parameters is not None and int(parameters.par_line_confidence_mode) != LINE_CONF_OFF:
        raise ValueError("%s: par_line_confidence_mode=%d together with u_dilation=%d is not built (the line confidence "
                         "takes no slope factor)" % (who, int(parameters.par_line_confidence_mode), u_dilation))


def _dilated_parameters(parameters: "Depth1DParameters", factor: int) -> "Depth1DParameters":
    """A copy of the parameters for the dilated frame: slope factor float32(par_slope_factor) * float32(factor).  The
    caller's object is not modified."""
    p = copy.copy(parameters)
    p.par_slope_factor = float(np.float32(parameters.par_slope_factor) * np.float32(factor))
    return p


def _level_dilation(level_dilation, level_dilation_kind, who: str) -> tuple[int, int]:
    """(factor, kind) of the level_dilation / level_dilation_kind arguments of the pyramid forms: an integer in 1..8, a
    DILATE_*."""
    f = 1 if level_dilation is None else level_dilation
    if isinstance(f, (bool, np.bool_)) or not isinstance(f, (int, np.integer)) or not 1 <= int(f) <= DILATE_MAX_FACTOR:
        raise ValueError("%s: level_dilation %r is not an integer in 1..%d" % (who, level_dilation, DILATE_MAX_FACTOR))
    if isinstance(level_dilation_kind, (bool, np.bool_)) or level_dilation_kind not in (DILATE_LINEAR, DILATE_CUBIC, DILATE_LANCZOS3):
        raise ValueError("%s: level_dilation_kind %r is not DILATE_LINEAR, DILATE_CUBIC or DILATE_LANCZOS3" % (who, level_dilation_kind))
    return int(f), int(level_dilation_kind)


def require_no_level_dilation(level_dilation, who: str) -> None:
    """The level dilation (DESIGN.md 3 "K18") is built for one device: fine_to_coarse_run_host and FineToCoarse.  A
    multi-device or sharded form would have to dilate every chunk of every level: they refuse it instead of ignoring it."""
    if level_dilation is not None and level_dilation != 1:
        raise ValueError("%s: level_dilation=%r is not built here (one device: fine_to_coarse_run_host, FineToCoarse)"
                         % (who, level_dilation))


def require_no_line_confidence_level_dilated(line_mode, level_dilation: int, who: str) -> None:
    """K7 samples C_e along u + (s_hat - s) * d with no slope factor (core.hpp:1058): in a level's dilated frame it would
    walk the wrong line."""
    if level_dilation != 1 and line_mode is not None and int(line_mode) != LINE_CONF_OFF:
        raise ValueError("%s: line confidence mode %d together with level_dilation=%d is not built (the line confidence takes "
                         "no slope factor)" % (who, int(line_mode), level_dilation))


def _derivative_weight(derivative_channels, who: str) -> float:
    """The weight of a derivative_channels argument: None, False or 0 is off (0.0); anything else is a finite weight > 0."""
    if derivative_channels is None or derivative_channels is False or derivative_channels == 0:
        return 0.0
    try:
        w = float(derivative_channels)
    except (TypeError, ValueError):
        w = float("nan")
    if isinstance(derivative_channels, bool) or not np.isfinite(w) or w <= 0 or w > float(np.finfo(np.float32).max):
        raise ValueError("%s: derivative_channels %r is not 0 (off) or a finite weight > 0" % (who, derivative_channels))
    return w


def require_no_derivative_channels(derivative_channels, who: str) -> None:
    """The derivative channels (DESIGN.md 3 "K17") are built for one device: the pyramid of fine_to_coarse_run_host and
    FineToCoarse, and Volume.with_derivative_channels for the three computers.  A multi-device or sharded form would have to
    exchange the rows v - 1 and v + 1 of every chunk's ends: they refuse it instead of ignoring it."""
    if derivative_channels is not None and derivative_channels is not False and derivative_channels != 0:
        raise ValueError("%s: derivative_channels=%r is not built here (one device: fine_to_coarse_run_host, FineToCoarse; or "
                         "Volume.with_derivative_channels)" % (who, derivative_channels))


EQUALIZE_GAIN, EQUALIZE_AFFINE = 1, 2   # RSLF_EQUALIZE_*


class ViewStats(NamedTuple):
    """Volume.view_stats(): per view and channel, [S, C] each -- the samples counted (uint64), and the mean and standard
    deviation of the quantised samples on the volume's own scale (float64; NaN where n == 0).  `raw` [S, C, 3] holds the
    integers (n, s1, s2) themselves and `hi` the cap they were quantised with (csrc/k19_equalize_rule.hpp)."""
    n: np.ndarray
    mean: np.ndarray
    std: np.ndarray
    raw: np.ndarray
    hi: float


def _equalize_mode(equalize_views, who: str) -> int:
    """The mode of an equalize_views argument: None, False or 0 is off (0); else EQUALIZE_GAIN or EQUALIZE_AFFINE."""
    if equalize_views is None or equalize_views is False or (not isinstance(equalize_views, str) and equalize_views == 0):
        return 0
    if isinstance(equalize_views, (bool, np.bool_)) or equalize_views not in (EQUALIZE_GAIN, EQUALIZE_AFFINE):
        raise ValueError("%s: equalize_views %r is not None (off), EQUALIZE_GAIN or EQUALIZE_AFFINE" % (who, equalize_views))
    return int(equalize_views)


def _equalize_args(S: int, C_: int, ref_view, joint, max_gain, who: str) -> tuple[int, int, float]:
    """(ref_view, joint, max_gain) as the library takes them.  ref_view None: the view S // 2, where the sweep starts;
    "mean": -1, the mean of the views; joint None: on for three channels."""
    if ref_view is None:
        ref = S // 2
    elif isinstance(ref_view, str):
        if ref_view != "mean":
            raise ValueError("%s: equalize ref_view %r is not None, \"mean\" or a view in [0, %d)" % (who, ref_view, S))
        ref = -1
    else:
        ref = int(ref_view)
        if isinstance(ref_view, (bool, np.bool_)) or ref != ref_view or not 0 <= ref < S:
            raise ValueError("%s: equalize ref_view %r is not None, \"mean\" or a view in [0, %d)" % (who, ref_view, S))
    j = (C_ == 3) if joint is None else bool(joint)
    if j and C_ != 3:
        raise ValueError("%s: equalize joint=%r needs a three-channel field, not C=%d" % (who, joint, C_))
    try:
        g = float(max_gain)
    except (TypeError, ValueError):
        g = float("nan")
    if isinstance(max_gain, bool) or not np.isfinite(g) or g < 1.0 or g > float(np.finfo(np.float32).max):
        raise ValueError("%s: equalize max_gain %r is not a finite gain >= 1" % (who, max_gain))
    return ref, 1 if j else 0, g


def require_no_equalize_views(equalize_views, who: str) -> None:
    """The per-view equalisation (DESIGN.md 3 "K19") is built for one device: a view's statistic spans all scanlines, so a
    multi-device or sharded form needs an all-reduce.  They refuse it instead of ignoring it."""
    if equalize_views is not None and equalize_views is not False and (isinstance(equalize_views, str) or equalize_views != 0):
        raise ValueError("%s: equalize_views=%r is not built here (one device: fine_to_coarse_run_host, FineToCoarse; or "
                         "Volume.equalized_views)" % (who, equalize_views))


class Context:
    """rslf_ctx bound to one GPU; launches go to torch's current stream on it."""

    def __init__(self, device: int | torch.device | None = None):
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        h = C.c_void_p()
        check(_lib.lib().rslf_ctx_create(self.device.index or 0, C.byref(h)), "rslf_ctx_create")
        self._h = h
        self.use_current_stream()

    def use_current_stream(self) -> None:
        s = torch.cuda.current_stream(self.device).cuda_stream
        check(_lib.lib().rslf_ctx_set_stream(self._h, C.c_void_p(s)), "rslf_ctx_set_stream")

    def synchronize(self) -> None:
        check(_lib.lib().rslf_ctx_synchronize(self._h), "rslf_ctx_synchronize")

    _DEBUG_DEFAULTS = dict(force_scan=0, force_groups=0, force_packed=-1, px=-1, stream_share=1, stream_groups=0, stream_lds_kib=80,
                           claim_skip=1, time_all=0, row_split=1, staging_kib=0, tap_table=1, scalar_taps=1,
                           subgrid_list=1, peaks_list=1, consistency_order=0)   # = the library's own defaults (rslf_internal.hpp, plan::kStreamLdsBytes)
    _FORCE_SCAN = {None: 0, "auto": 0, "generic": 1, "stream": 2}

    def set_debug(self, **hooks) -> None:
        """rslf_ctx_set_debug: test / tuning hooks of THIS context (kernel variant, launch shape).  force_scan also
        takes "generic" / "stream" / None."""
        for k, v in hooks.items():
            if k == "force_scan" and not isinstance(v, int):
                v = self._FORCE_SCAN[v or None]
            check(_lib.lib().rslf_ctx_set_debug(self._h, k.encode(), int(v)), "rslf_ctx_set_debug(%s)" % k)

    def reset_debug(self) -> None:
        self.set_debug(**self._DEBUG_DEFAULTS)

    def last_scan_kernel_ms(self) -> float:
        ms = C.c_float()
        check(_lib.lib().rslf_last_scan_kernel_ms(self._h, C.byref(ms)), "rslf_last_scan_kernel_ms")
        return float(ms.value)

    def last_scan_row_exact(self) -> tuple[bool, int]:
        """(the last scan's launch was handed a row-exact table, row-exact hypotheses in it): rslf_last_scan_row_exact."""
        a, n = C.c_int(), C.c_int()
        check(_lib.lib().rslf_last_scan_row_exact(self._h, C.byref(a), C.byref(n)), "rslf_last_scan_row_exact")
        return bool(a.value), int(n.value)

    def scan_time_total_ms(self) -> tuple[float, int]:
        """With set_debug(time_all=1): (summed K2 milliseconds, scan launches) since the last call; resets the sum."""
        ms, n = C.c_float(), C.c_int()
        check(_lib.lib().rslf_scan_time_total_ms(self._h, C.byref(ms), C.byref(n)), "rslf_scan_time_total_ms")
        return float(ms.value), int(n.value)

    def get_withheld_sources(self) -> int:
        """rslf_sweep_withheld: the sources the last finished 2-D sweep on this context withheld from propagation
        (propagation_ratio); 0 if it had no ratio.  Waits for the stream."""
        n = C.c_ulonglong()
        check(_lib.lib().rslf_sweep_withheld(self._h, C.byref(n)), "rslf_sweep_withheld")
        return int(n.value)

    def close(self) -> None:
        # at interpreter shutdown the HIP runtime may already be gone: leave the handle to the OS
        if getattr(self, "_h", None) and not sys.is_finalizing():
            _lib.lib().rslf_ctx_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


_DEFAULT_CTX: dict[int, Context] = {}


@atexit.register
def _drop_default_contexts() -> None:
    # release while the HIP runtime is still alive (module globals die too late for that)
    for c in list(_DEFAULT_CTX.values()):
        c._h = None
    _DEFAULT_CTX.clear()


def default_context(device=None) -> Context:
    idx = torch.cuda.current_device() if device is None else torch.device(device).index or 0
    if idx not in _DEFAULT_CTX:
        _DEFAULT_CTX[idx] = Context(idx)
    return _DEFAULT_CTX[idx]


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


# The element types of a host light field (the reference's CV_8U, CV_16U and CV_32F Mats) and their C-ABI suffixes.
_SUFFIX = {np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16", np.dtype(np.float32): "f32"}


def field_dtype(dtype) -> np.dtype:
    """The element type a host light field of `dtype` is sent as: uint8 and uint16 as they are, anything else as float32
    (the reference's constructors normalise every depth other than 8U by the max, dc.hpp:269-288, :442-475, :671-705)."""
    dt = np.dtype(dtype)
    return dt if dt in (np.uint8, np.uint16) else np.dtype(np.float32)


class Volume:
    """The light-field slab in HBM, [V][S][pitch][C] float32 (rslf_volume)."""

    def __init__(self, ctx: Context, V: int, S: int, U: int, C_: int):
        self.ctx = ctx
        h = C.c_void_p()
        check(_lib.lib().rslf_volume_create(ctx._h, V, S, U, C_, C.byref(h)), "rslf_volume_create")
        self._h = h
        self.V, self.S, self.U, self.C = V, S, U, C_
        self.scale_used: float | None = None
        self.u_dilation = 1                    # of a volume dilated_u() made: the factor ...
        self.u_source: Volume | None = None    # ... and the volume it was made from
        self.derivative_weight = 0.0           # of a volume with_derivative_channels() made: the weight

    # -- constructors -----------------------------------------------------
    @staticmethod
    def from_epis(epis: Sequence[np.ndarray], epi_scale_factor: float = -1.0, ctx: Context | None = None) -> "Volume":
        """The reference's constructor input: a Vec<Mat> of V EPIs, each [S,U] or
        [S,U,3], uint8, uint16 or float32 (dc.hpp:425-477).  uint16 goes up as it is (no host cast) and is
        normalised like float: by the max over all values unless a factor is given."""
        ctx = ctx or default_context()
        e0 = np.asarray(epis[0])
        S, U = e0.shape[:2]
        C_ = 1 if e0.ndim == 2 else e0.shape[2]
        vol = Volume(ctx, len(epis), S, U, C_)
        dt = field_dtype(e0.dtype)
        arrs, ptrs, stride = host_rows(epis, dt)   # (arrs: alive over the calls below)
        L = _lib.lib()
        ctx.use_current_stream()
        if dt == np.uint8:
            check(L.rslf_volume_upload_epis_u8(vol._h, ptrs, stride), "rslf_volume_upload_epis_u8")
            vol.scale_used = 255.0
        else:
            name = "rslf_volume_upload_epis_" + _SUFFIX[dt]
            su = C.c_float()
            check(getattr(L, name)(vol._h, ptrs, stride, float(epi_scale_factor), C.byref(su)), name)
            vol.scale_used = float(su.value)
        return vol

    @staticmethod
    def from_images(imgs: Sequence[np.ndarray], epi_scale_factor: float = -1.0, ctx: Context | None = None,
                    transpose: bool = False, rotate_180: bool = False) -> "Volume":
        """Image-major input, images each [V,U] or [V,U,3] -- what rslf::build_epis_from_imgs
        (rslf_io.cpp:194-227) consumes, with its `transpose` / `rotate_180` options: transposed, the EPI of a
        scanline has one row per image COLUMN and one column per image."""
        ctx = ctx or default_context()
        i0 = np.asarray(imgs[0])
        V, cols = i0.shape[:2]
        C_ = 1 if i0.ndim == 2 else i0.shape[2]
        S, U = (cols, len(imgs)) if transpose else (len(imgs), cols)
        vol = Volume(ctx, V, S, U, C_)
        dt = field_dtype(i0.dtype)
        arrs, ptrs, stride = host_rows(imgs, dt)   # (arrs: alive over the calls below)
        L = _lib.lib()
        ctx.use_current_stream()
        plain = not (transpose or rotate_180)
        if dt == np.uint8:
            if plain:
                check(L.rslf_volume_upload_images_u8(vol._h, ptrs, stride), "rslf_volume_upload_images_u8")
            else:
                check(L.rslf_volume_upload_images_xf_u8(vol._h, ptrs, stride, int(transpose), int(rotate_180)),
                      "rslf_volume_upload_images_xf_u8")
            vol.scale_used = 255.0
        else:
            su = C.c_float()
            if plain:
                name = "rslf_volume_upload_images_" + _SUFFIX[dt]
                check(getattr(L, name)(vol._h, ptrs, stride, float(epi_scale_factor), C.byref(su)), name)
            else:
                name = "rslf_volume_upload_images_xf_" + _SUFFIX[dt]
                check(getattr(L, name)(vol._h, ptrs, stride, float(epi_scale_factor), C.byref(su), int(transpose), int(rotate_180)), name)
            vol.scale_used = float(su.value)
        return vol

    @staticmethod
    def from_dense(vsuc, epi_scale_factor: float = 1.0, ctx: Context | None = None) -> "Volume":
        """Dense [V,S,U] / [V,S,U,C] float32, numpy (uploaded) or a CUDA tensor
        (packed on the device)."""
        ctx = ctx or default_context()
        if isinstance(vsuc, np.ndarray):
            a = np.ascontiguousarray(vsuc, np.float32)
            if a.ndim == 4 and a.shape[3] == 1:
                a = a[..., 0]
            return Volume.from_epis(list(a), epi_scale_factor, ctx)
        t = vsuc
        if t.dim() == 3:
            t = t.unsqueeze(-1)
        if not t.is_cuda or t.dtype != torch.float32:
            raise ValueError("from_dense needs a float32 CUDA tensor or a numpy array")
        t = t.contiguous()
        V, S, U, C_ = t.shape
        vol = Volume(ctx, V, S, U, C_)
        ctx.use_current_stream()
        su = C.c_float()
        check(_lib.lib().rslf_volume_pack_device_f32(vol._h, _ptr(t), float(epi_scale_factor), C.byref(su)),
              "rslf_volume_pack_device_f32")
        vol.scale_used = float(su.value)
        return vol

    def dilated_u(self, factor: int, kind: int = DILATE_CUBIC) -> "Volume":
        """Not in the reference's code (its report's fourth lead): a new Volume resampled along u by the integer `factor`
        (1..8) with the kernel `kind` (DILATE_*), U' = factor * (U - 1) + 1 columns wide (rslf_volume_dilate_u).  Column
        i * factor holds this volume's column i bit for bit; min and max are this volume's.  Run any path on it with
        par_slope_factor * factor.  The result carries .u_dilation and .u_source."""
        factor, kind = _u_dilation(factor, kind, "Volume.dilated_u")
        self.ctx.use_current_stream()
        h = C.c_void_p()
        check(_lib.lib().rslf_volume_dilate_u(self.ctx._h, self._h, factor, kind, C.byref(h)), "rslf_volume_dilate_u")
        out = Volume.__new__(Volume)
        out.ctx, out._h = self.ctx, h
        out.V, out.S, out.U, out.C = self.V, self.S, factor * (self.U - 1) + 1, self.C
        out.scale_used = self.scale_used
        out.u_dilation, out.u_source = factor, self
        out.derivative_weight = self.derivative_weight
        return out

    def with_derivative_channels(self, weight: float) -> "Volume":
        """Not in the reference's code (its report's second lead): a new three-channel Volume (x, fu, fv) from this
        one-channel one, fu = min(|x[u+1] - x[u-1]| * weight / 2, hi) along u and fv the same along v, neighbours clamped
        to the field, hi = max(max_value, 0) (rslf_volume_derivative_channels).  Channel 0 holds this volume's bits and the
        maximum is this volume's.  Any computer takes the result as it takes a three-channel Volume.  The result carries
        .derivative_weight."""
        w = _derivative_weight(weight, "Volume.with_derivative_channels")
        if w == 0.0:
            raise ValueError("Volume.with_derivative_channels: derivative_channels %r is not a finite weight > 0" % (weight,))
        self.ctx.use_current_stream()
        h = C.c_void_p()
        check(_lib.lib().rslf_volume_derivative_channels(self.ctx._h, self._h, w, C.byref(h)), "rslf_volume_derivative_channels")
        out = Volume.__new__(Volume)
        out.ctx, out._h = self.ctx, h
        out.V, out.S, out.U, out.C = self.V, self.S, self.U, 3
        out.scale_used = self.scale_used
        out.u_dilation, out.u_source = self.u_dilation, self.u_source
        out.derivative_weight = w
        return out

    view_gains = None   # of a volume equalized_views() / with_view_gains() made: the [S, C, 2] float32 (a, b) it was made with

    def _require_intensities(self, who: str) -> None:
        if getattr(self, "derivative_weight", 0.0) > 0:
            raise ValueError("%s: a volume with derivative channels (derivative_weight=%r) is refused: its feature channels are "
                             "not intensities; equalise first" % (who, self.derivative_weight))

    def _like(self, h) -> "Volume":
        """A new Volume of this one's shape around the handle h, with what this one carries."""
        out = Volume.__new__(Volume)
        out.ctx, out._h = self.ctx, h
        out.V, out.S, out.U, out.C = self.V, self.S, self.U, self.C
        out.scale_used = self.scale_used
        out.u_dilation, out.u_source = self.u_dilation, self.u_source
        out.derivative_weight = self.derivative_weight
        return out

    def view_stats(self) -> ViewStats:
        """Not in the reference's code: per view and channel, over all (v, u), the count, mean and standard deviation of
        this volume's samples quantised to 16 bits of [0, max_value] (rslf_volume_view_stats) -- integers, so the same bits
        on every run.  A non-negative volume with a finite maximum > 0."""
        self._require_intensities("Volume.view_stats")
        raw = np.zeros((self.S, self.C, 3), np.uint64)
        hi = C.c_float()
        self.ctx.use_current_stream()
        check(_lib.lib().rslf_volume_view_stats(self.ctx._h, self._h, raw.ctypes.data, C.byref(hi)), "rslf_volume_view_stats")
        n = raw[..., 0].copy()
        with np.errstate(invalid="ignore", divide="ignore"):
            dn = n.astype(np.float64)
            h = float(hi.value)
            mean = raw[..., 1].astype(np.float64) / dn / 65535.0 * h
            var = raw[..., 2].astype(np.float64) / dn / (65535.0 * 65535.0) * (h * h) - mean * mean
            std = np.sqrt(np.maximum(var, 0.0))
        return ViewStats(n, mean, std, raw, h)

    def equalized_views(self, mode: int = EQUALIZE_AFFINE, ref_view=None, joint=None, max_gain: float = 4.0) -> "Volume":
        """Not in the reference's code (the remedy its report names for global changes of illumination between frames): a
        new Volume y = a x + b with one (a, b) per view and channel, so that every view's mean (EQUALIZE_GAIN: b = 0) or mean
        and standard deviation (EQUALIZE_AFFINE) over all (v, u) meet the reference view's (rslf_volume_equalize_views).
        ref_view None: the view S // 2, where the sweep starts; "mean": the mean of the views.  joint None: one pair for
        the three channels of an RGB volume (hue is kept), False: a pair per channel.  The gain is clamped to
        [1 / max_gain, max_gain].  The result carries .view_gains [S, C, 2] and what this volume carries."""
        m = _equalize_mode(mode, "Volume.equalized_views")
        if m == 0:
            raise ValueError("Volume.equalized_views: equalize_views %r is not EQUALIZE_GAIN or EQUALIZE_AFFINE" % (mode,))
        self._require_intensities("Volume.equalized_views")
        ref, j, g = _equalize_args(self.S, self.C, ref_view, joint, max_gain, "Volume.equalized_views")
        a_b = np.zeros((self.S, self.C, 2), np.float32)
        self.ctx.use_current_stream()
        h = C.c_void_p()
        check(_lib.lib().rslf_volume_equalize_views(self.ctx._h, self._h, m, ref, j, g, C.byref(h), a_b.ctypes.data),
              "rslf_volume_equalize_views")
        out = self._like(h)
        out.view_gains = a_b
        return out

    def with_view_gains(self, a_b) -> "Volume":
        """The apply pass alone (rslf_volume_apply_view_gains): a new Volume y = a x + b from the caller's [S, C, 2]
        coefficients -- a masked statistic of their own, another field's gains.  y is rounded as the rule says and clamped
        to [0, max_value]; a pair (1, 0) copies the view."""
        self._require_intensities("Volume.with_view_gains")
        t = np.ascontiguousarray(a_b, np.float32)
        if t.shape != (self.S, self.C, 2) or not np.isfinite(t).all():
            raise ValueError("Volume.with_view_gains: view_gains must be finite and [S, C, 2] = %s, not %s"
                             % ((self.S, self.C, 2), t.shape))
        self.ctx.use_current_stream()
        h = C.c_void_p()
        check(_lib.lib().rslf_volume_apply_view_gains(self.ctx._h, self._h, t.ctypes.data, C.byref(h)), "rslf_volume_apply_view_gains")
        out = self._like(h)
        out.view_gains = t.copy()
        return out

    def describe(self) -> RslfVolumeDesc:
        d = RslfVolumeDesc()
        check(_lib.lib().rslf_volume_describe(self._h, C.byref(d)), "rslf_volume_describe")
        return d

    def close(self) -> None:
        if getattr(self, "_h", None) and not sys.is_finalizing():
            _lib.lib().rslf_volume_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def undilate_u(ctx: Context, planes: torch.Tensor, factor: int) -> torch.Tensor:
    """Result planes of a dilated frame on the source grid: planes[..., ::factor] as a new dense tensor, on the device
    (rslf_planes_undilate_u).  Any leading dimensions; uint8, float32 or int32 CUDA tensors whose last dimension is
    factor * (U - 1) + 1."""
    factor, _ = _u_dilation(factor, DILATE_CUBIC, "undilate_u")
    if not planes.is_cuda or planes.dtype not in (torch.uint8, torch.float32, torch.int32):
        raise ValueError("undilate_u needs a uint8, float32 or int32 CUDA tensor")
    if planes.dim() < 1 or planes.shape[-1] < 1 or (planes.shape[-1] - 1) % factor != 0:
        raise ValueError("undilate_u: the last dimension %s is not factor * (U - 1) + 1 for factor=%d"
                         % (planes.shape[-1] if planes.dim() else None, factor))
    t = planes.contiguous()
    Ud = t.shape[-1]
    out = torch.empty(tuple(t.shape[:-1]) + ((Ud - 1) // factor + 1,), dtype=t.dtype, device=t.device)
    ctx.use_current_stream()
    check(_lib.lib().rslf_planes_undilate_u(ctx._h, _ptr(t), t.element_size(), t.numel() // Ud, Ud, factor, _ptr(out)),
          "rslf_planes_undilate_u")
    return out


def undilate_many_u(ctx: Context, planes: Sequence[torch.Tensor], factor: int) -> list:
    """undilate_u for several planes of the same shape in ONE launch (rslf_planes_undilate_many_u): at most 8 float32 /
    int32 and 2 uint8 CUDA tensors, any leading dimensions, last dimension factor * (U - 1) + 1.  Returns new dense tensors
    in the planes' order."""
    factor, _ = _u_dilation(factor, DILATE_CUBIC, "undilate_many_u")
    planes = list(planes)
    if not planes:
        raise ValueError("undilate_many_u: no planes")
    shape = tuple(planes[0].shape)
    for t in planes:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.uint8, torch.float32, torch.int32):
            raise ValueError("undilate_many_u needs uint8, float32 or int32 CUDA tensors")
        if tuple(t.shape) != shape:
            raise ValueError("undilate_many_u: planes of different shapes, %s and %s" % (shape, tuple(t.shape)))
    if len(shape) < 1 or shape[-1] < 1 or (shape[-1] - 1) % factor != 0:
        raise ValueError("undilate_many_u: the last dimension %s is not factor * (U - 1) + 1 for factor=%d"
                         % (shape[-1] if shape else None, factor))
    n4, n1 = sum(t.element_size() == 4 for t in planes), sum(t.element_size() == 1 for t in planes)
    if n4 > 8 or n1 > 2:
        raise ValueError("undilate_many_u: %d planes of 4-byte and %d of 1-byte elements: at most 8 and 2 in one call" % (n4, n1))
    src = [t.contiguous() for t in planes]
    Ud = shape[-1]
    outs = [torch.empty(shape[:-1] + ((Ud - 1) // factor + 1,), dtype=t.dtype, device=t.device) for t in src]
    n = len(src)
    ctx.use_current_stream()
    check(_lib.lib().rslf_planes_undilate_many_u(ctx._h, (C.c_void_p * n)(*[t.data_ptr() for t in src]),
                                                 (C.c_void_p * n)(*[t.data_ptr() for t in outs]),
                                                 (C.c_int * n)(*[t.element_size() for t in src]), n, src[0].numel() // Ud, Ud, factor),
          "rslf_planes_undilate_many_u")
    return outs


def dilate_ranges_u(ctx: Context, dmin: torch.Tensor, dmax: torch.Tensor, factor: int) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-pixel hypothesis ranges [..., U] in the frame dilated along u, [..., factor * (U - 1) + 1], on the device
    (rslf_planes_dilate_ranges_u, K18): column i * factor takes column i's range bit for bit, the columns between i and
    i + 1 the union of the two neighbours' ranges.  float32 CUDA tensors of one shape."""
    factor, _ = _u_dilation(factor, DILATE_CUBIC, "dilate_ranges_u")
    for t in (dmin, dmax):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise ValueError("dilate_ranges_u needs float32 CUDA tensors")
    if tuple(dmin.shape) != tuple(dmax.shape) or dmin.dim() < 1 or dmin.shape[-1] < 1:
        raise ValueError("dilate_ranges_u: dmin %s and dmax %s are not two planes of one shape" % (tuple(dmin.shape), tuple(dmax.shape)))
    lo, hi = dmin.contiguous(), dmax.contiguous()
    U = lo.shape[-1]
    shape = tuple(lo.shape[:-1]) + (factor * (U - 1) + 1,)
    out_lo, out_hi = torch.empty(shape, dtype=torch.float32, device=lo.device), torch.empty(shape, dtype=torch.float32, device=lo.device)
    ctx.use_current_stream()
    check(_lib.lib().rslf_planes_dilate_ranges_u(ctx._h, _ptr(lo), _ptr(hi), lo.numel() // U, U, factor, _ptr(out_lo), _ptr(out_hi)),
          "rslf_planes_dilate_ranges_u")
    return out_lo, out_hi


def _undilated(who: str, planes: dict, name: str, vol: "Volume", channels_last=()) -> torch.Tensor:
    """The plane `name` of a computer's members on the source grid (the `undilated` getters)."""
    if name not in planes:
        raise ValueError("%s.undilated: no plane %r (one of %s)" % (who, name, ", ".join(sorted(planes))))
    t = planes[name]
    if t is None:
        raise ValueError("%s.undilated: the plane %r is not held by this object" % (who, name))
    if vol.u_dilation == 1:
        return t
    if name in channels_last:   # [..., U', C]: the columns are the last dimension but one
        return undilate_u(vol.ctx, t.movedim(-1, 0), vol.u_dilation).movedim(0, -1).contiguous()
    return undilate_u(vol.ctx, t, vol.u_dilation)


# ---- rendering: the getters' pictures (include/rslf_hip.h, "rendering"; csrc/k6_render.hpp) ----------------------

FIT_MINMAX, FIT_QUANTILE, FIT_MEANSTD = 0, 1, 2      # RSLF_FIT_*
RENDER_SHIFT, RENDER_AFFINE = 0, 1                   # RSLF_RENDER_*
MASK_BLACK, MASK_ZERO_VALUE = 0, 1                   # RSLF_MASK_*
SLICE_VIEW, SLICE_EPI = 0, 1                         # RSLF_SLICE_*


def colormap_jet() -> np.ndarray:
    """A jet table [256, 3] uint8, BGR, for the getters' `lut_bgr`.  Restated from memory of OpenCV 3.4, unpinned: the
    library knows no colour map by name (cv::applyColorMap lives in OpenCV, not in the reference), no test compares
    this table with OpenCV's COLORMAP_JET, and none may rest on it.  Any [256, 3] uint8 table serves instead."""
    x = np.arange(256, dtype=np.float64) / 255.0
    r = np.clip(1.5 - np.abs(4.0 * x - 3.0), 0.0, 1.0)
    g = np.clip(1.5 - np.abs(4.0 * x - 2.0), 0.0, 1.0)
    b = np.clip(1.5 - np.abs(4.0 * x - 1.0), 0.0, 1.0)
    return np.rint(np.stack([b, g, r], axis=1) * 255.0).astype(np.uint8)


def _table(lut_bgr) -> np.ndarray:
    t = colormap_jet() if lut_bgr is None else np.ascontiguousarray(lut_bgr)
    if t.dtype != np.uint8 or t.shape != (256, 3):
        raise ValueError("lut_bgr must be a [256, 3] uint8 array (level i -> lut_bgr[i], BGR)")
    return t


def _strided(t: torch.Tensor, like: torch.Tensor | None = None) -> tuple:
    """Strides in elements of a plane stack whose rows are contiguous (views of larger stacks are taken as they are)."""
    if not t.is_cuda or t.stride(-1) != 1 and t.shape[-1] > 1:
        raise ValueError("planes must be CUDA tensors with contiguous rows")
    if like is not None and (t.shape != like.shape or t.stride() != like.stride()):
        raise ValueError("the mask must have the planes' shape and strides")
    return t.stride()


def _index_rule(name: str, *args) -> int:
    """The getters' two index rules (rslf_render_centre_index / rslf_render_scaled_row): ValueError where the
    reference's own index runs off the end."""
    out = C.c_int()
    st = getattr(_lib.lib(), name)(*args, C.byref(out))
    if st == -1:
        raise ValueError(_lib.lib().rslf_last_error().decode(errors="replace"))
    check(st, name)
    return int(out.value)


def render_fit(ctx: Context, plane: torch.Tensor, valid: torch.Tensor | None = None, mode: int = FIT_MINMAX) -> tuple[float, float]:
    """rslf_render_fit: the (min, max) a converter holds for a [rows, cols] float32 plane (a strided slice of a stack
    is fine).  mode FIT_MINMAX: cv::minMaxLoc; FIT_QUANTILE: ImageConverter_uchar::fit(img, true), elements
    floor(0.02 N) and floor(0.98 N) of the sort; FIT_MEANSTD: fit(img, false).  `valid` (uint8, same shape and strides): a
    pixel whose byte is 0 counts as 0.  Waits for the result.  What a NaN in the plane gives is unspecified."""
    if plane.dim() != 2 or plane.dtype != torch.float32 or (valid is not None and valid.dtype != torch.uint8):
        raise ValueError("render_fit takes a 2-D float32 plane and a uint8 mask")
    stride = _strided(plane)
    if valid is not None:
        _strided(valid, plane)
    rows, cols = plane.shape
    lo, hi = C.c_double(), C.c_double()
    ctx.use_current_stream()
    check(_lib.lib().rslf_render_fit(ctx._h, _ptr(plane), rows, cols, stride[0] if rows > 1 else cols, _ptr(valid), int(mode),
                                     C.byref(lo), C.byref(hi)), "rslf_render_fit")
    return float(lo.value), float(hi.value)


def render_planes(ctx: Context, planes: torch.Tensor, vmin: float, vmax: float, formula: int, lut_bgr, valid: torch.Tensor | None = None,
                  mask_mode: int = MASK_BLACK, vol: "Volume | None" = None, slice_kind: int = SLICE_VIEW, index: int = 0,
                  shadow_level: float = 0.0) -> torch.Tensor:
    """rslf_render_planes: [n, rows, cols] float32 planes (strided slices are fine) -> [n, rows, cols, 3] uint8 BGR in one
    launch.  Level by `formula` (RENDER_SHIFT: copy_and_scale_uchar; RENDER_AFFINE: ImageConverter_uchar::copy_and_scale)
    from (vmin, vmax), then lut_bgr, then `valid` by `mask_mode` (MASK_BLACK: black where the byte is 0; MASK_ZERO_VALUE:
    the value counts as 0 before the level is taken), then with `vol` the shadow cut: black where the norm of the
    volume's radiance is below shadow_level (SLICE_VIEW: plane k is view index + k; SLICE_EPI: the one plane is scanline
    `index`, its rows are views).  What a NaN in a plane renders as is unspecified."""
    if planes.dim() != 3 or planes.dtype != torch.float32 or (valid is not None and valid.dtype != torch.uint8):
        raise ValueError("render_planes takes 3-D float32 planes and a uint8 mask")
    stride = _strided(planes)
    if valid is not None:
        _strided(valid, planes)
    n, rows, cols = planes.shape
    table = _table(lut_bgr)
    out = torch.empty((n, rows, cols, 3), dtype=torch.uint8, device=planes.device)
    ctx.use_current_stream()
    check(_lib.lib().rslf_render_planes(
        ctx._h, _ptr(planes), n, stride[0] if n > 1 else 0, rows, cols, stride[1] if rows > 1 else cols, float(vmin), float(vmax),
        int(formula), table.ctypes.data_as(C.c_void_p), _ptr(valid), int(mask_mode), vol._h if vol is not None else None,
        int(slice_kind), int(index), float(shadow_level), _ptr(out)), "rslf_render_planes")
    return out


def _stack_args(planes: torch.Tensor, valid: torch.Tensor | None, who: str) -> tuple:
    """(n, plane_stride, rows, cols, row_stride) of a [n, rows, cols] float32 stack read in place, as the C entries take it."""
    if planes.dim() != 3 or planes.dtype != torch.float32 or (valid is not None and valid.dtype != torch.uint8):
        raise ValueError("%s takes 3-D float32 planes and a uint8 mask" % who)
    stride = _strided(planes)
    if valid is not None:
        _strided(valid, planes)
    n, rows, cols = planes.shape
    return n, stride[0] if n > 1 else 0, rows, cols, stride[1] if rows > 1 else cols


def render_fit_many(ctx: Context, planes: torch.Tensor, valid: torch.Tensor | None = None, mode: int = FIT_MINMAX) -> list:
    """rslf_render_fit_many: render_fit for every plane of a [n, rows, cols] float32 stack (n <= 65535) -> a list of n
    (min, max), each bit for bit render_fit's for that plane alone, in launches whose number does not depend on n, one
    copy and one wait.  The stack is read in place through its strides: depth_s_v_u for every view,
    depth_s_v_u.permute(1, 0, 2) for every EPI slice.  `valid`: uint8, same shape and strides."""
    n, plane_stride, rows, cols, row_stride = _stack_args(planes, valid, "render_fit_many")
    out = (C.c_double * (2 * max(n, 1)))()
    ctx.use_current_stream()
    check(_lib.lib().rslf_render_fit_many(ctx._h, _ptr(planes), n, plane_stride, rows, cols, row_stride, _ptr(valid), int(mode), out),
          "rslf_render_fit_many")
    return [(float(out[2 * k]), float(out[2 * k + 1])) for k in range(n)]


def render_planes_each(ctx: Context, planes: torch.Tensor, minmax, formula: int, lut_bgr, valid: torch.Tensor | None = None,
                       mask_mode: int = MASK_BLACK, vol: "Volume | None" = None, slice_kind: int = SLICE_VIEW, index: int = 0,
                       shadow_level: float = 0.0) -> torch.Tensor:
    """rslf_render_planes_each: render_planes with plane k scaled over minmax[k] = (min, max) (as render_fit_many returns
    them) -> [n, rows, cols, 3] uint8 BGR in one launch.  With SLICE_EPI plane k is scanline index + k of `vol`."""
    n, plane_stride, rows, cols, row_stride = _stack_args(planes, valid, "render_planes_each")
    mm = np.ascontiguousarray(minmax, dtype=np.float64)
    if mm.shape != (n, 2):
        raise ValueError("minmax must hold one (min, max) per plane")
    table = _table(lut_bgr)
    out = torch.empty((n, rows, cols, 3), dtype=torch.uint8, device=planes.device)
    ctx.use_current_stream()
    check(_lib.lib().rslf_render_planes_each(
        ctx._h, _ptr(planes), n, plane_stride, rows, cols, row_stride, mm.ctypes.data_as(C.POINTER(C.c_double)), int(formula),
        table.ctypes.data_as(C.c_void_p), _ptr(valid), int(mask_mode), vol._h if vol is not None else None, int(slice_kind), int(index),
        float(shadow_level), _ptr(out)), "rslf_render_planes_each")
    return out


def render_epi_lines(ctx: Context, depth_v_u: torch.Tensor, mask_v_u: torch.Tensor, S: int, s_hat: int, v_first: int, n_rows: int,
                     lut_bgr) -> torch.Tensor:
    """rslf_render_epi_lines: the z-buffered EPI lines of get_coloured_epi for scanlines v_first .. v_first + n_rows - 1 of
    the [V, U] planes -> [n_rows, S, U, 3] uint8 BGR.  A NaN depth draws nothing."""
    if depth_v_u.dim() != 2 or depth_v_u.dtype != torch.float32 or mask_v_u.dtype != torch.uint8 or mask_v_u.shape != depth_v_u.shape:
        raise ValueError("render_epi_lines takes [V, U] float32 depths and a uint8 mask of the same shape")
    depth_v_u, mask_v_u = depth_v_u.contiguous(), mask_v_u.contiguous()
    V, U = depth_v_u.shape
    table = _table(lut_bgr)
    out = torch.empty((n_rows, S, U, 3), dtype=torch.uint8, device=depth_v_u.device)
    ctx.use_current_stream()
    check(_lib.lib().rslf_render_epi_lines(ctx._h, _ptr(depth_v_u), _ptr(mask_v_u), V, int(S), U, int(s_hat), int(v_first), int(n_rows),
                                           table.ctypes.data_as(C.c_void_p), _ptr(out)), "rslf_render_epi_lines")
    return out


def _coloured_epi_rows(ctx: Context, depth_v_u, mask_v_u, S: int, s_hat: int, a_v, lut_bgr) -> torch.Tensor:
    """get_coloured_epi's scanline argument: an int (< 0: floor(V / 2.0), dc.hpp:576-577) -> [S, U, 3]; a range of step 1 ->
    [len, S, U, 3], the same scanlines in one call."""
    V = depth_v_u.shape[0]
    if isinstance(a_v, range):
        if a_v.step != 1 or len(a_v) < 1 or a_v.start < 0 or a_v.stop > V:
            raise ValueError("a_v must be a non-empty range of step 1 within the %d scanlines" % V)
        return render_epi_lines(ctx, depth_v_u, mask_v_u, S, s_hat, a_v.start, len(a_v), lut_bgr)
    a_v = int(np.floor(V / 2.0)) if a_v < 0 else int(a_v)
    if a_v >= V:
        raise ValueError("scanline %d of %d" % (a_v, V))
    return render_epi_lines(ctx, depth_v_u, mask_v_u, S, s_hat, a_v, 1, lut_bgr)[0]


# ---- the reference's free functions -------------------------------------

def compute_1D_edge_confidence_pile(vol: Volume, a_s: int, a_edge_confidence_v_u: torch.Tensor,
                                    a_parameters: Depth1DParameters | None = None) -> torch.Tensor:
    """core.hpp:279-287.  Accumulates INTO a_edge_confidence_v_u ([V,U] f32
    CUDA, pass zeros) and returns the new mask ([V,U] u8) -- the reference
    allocates the mask itself (core.hpp:740)."""
    p = (a_parameters or Depth1DParameters()).to_c()
    mask = torch.empty((vol.V, vol.U), dtype=torch.uint8, device=a_edge_confidence_v_u.device)
    vol.ctx.use_current_stream()
    check(_lib.lib().rslf_edge_confidence_pile(vol.ctx._h, vol._h, a_s, C.byref(p), _ptr(a_edge_confidence_v_u), _ptr(mask)),
          "rslf_edge_confidence_pile")
    return mask


def compute_1D_depth_epi_pile(vol: Volume, a_dmin_v_u, a_dmax_v_u, a_dim_d: int, a_s_hat: int,
                              a_edge_confidence_v_u: torch.Tensor, a_edge_confidence_mask_v_u: torch.Tensor,
                              a_disp_confidence_v_u: torch.Tensor, a_best_depth_v_u: torch.Tensor,
                              a_rbar_v_u: torch.Tensor, a_parameters: Depth1DParameters | None = None,
                              a_mask_v_u: torch.Tensor | None = None, *, idx_v_u: torch.Tensor | None = None,
                              score_v_u: torch.Tensor | None = None, depth_raw_v_u: torch.Tensor | None = None,
                              want_stats: bool = False, a_K_r_m_rbar_v_s_u: torch.Tensor | None = None,
                              subgrid: bool = False) -> RslfStats | None:
    """core.hpp:293-310.  a_dmin_v_u / a_dmax_v_u are [V,U] f32 CUDA tensors or
    Python floats (the constant planes of dc.hpp:486-487).  All planes are
    updated in place; a_best_depth_v_u ends as the selective median (core.hpp:892).
    a_K_r_m_rbar_v_s_u ([V,S,U] f32, the reference's optional last argument, core.hpp:309): receives
    K(r - rbar)[:, d*] for every pixel that got a disparity (core.hpp:647-651).
    subgrid (not in the reference): every disparity the scan writes is moved off the hypothesis grid (subgrid_refine)
    before the median filters it; depth_raw_v_u then holds the refined, unfiltered plane."""
    p = (a_parameters or Depth1DParameters()).to_c()
    planes = isinstance(a_dmin_v_u, torch.Tensor)
    st = RslfStats() if want_stats else None
    vol.ctx.use_current_stream()
    if a_K_r_m_rbar_v_s_u is not None and idx_v_u is None:
        idx_v_u = torch.empty((vol.V, vol.U), dtype=torch.int32, device=a_best_depth_v_u.device)
    args = (vol.ctx._h, vol._h, _ptr(a_dmin_v_u if planes else None), _ptr(a_dmax_v_u if planes else None),
            0.0 if planes else float(a_dmin_v_u), 0.0 if planes else float(a_dmax_v_u), a_dim_d, a_s_hat,
            _ptr(a_edge_confidence_v_u), _ptr(a_edge_confidence_mask_v_u), _ptr(a_disp_confidence_v_u),
            _ptr(a_best_depth_v_u), _ptr(a_rbar_v_u), C.byref(p), _ptr(a_mask_v_u), _ptr(idx_v_u), _ptr(score_v_u),
            _ptr(depth_raw_v_u), C.byref(st) if st is not None else None)
    if subgrid:
        check(_lib.lib().rslf_depth_epi_pile_sub(*args, 1), "rslf_depth_epi_pile_sub")
    else:
        check(_lib.lib().rslf_depth_epi_pile(*args), "rslf_depth_epi_pile")
    if a_K_r_m_rbar_v_s_u is not None:
        check(_lib.lib().rslf_kernel_columns_pile(
            vol.ctx._h, vol._h, _ptr(a_dmin_v_u if planes else None), _ptr(a_dmax_v_u if planes else None),
            0.0 if planes else float(a_dmin_v_u), 0.0 if planes else float(a_dmax_v_u), a_dim_d, a_s_hat, C.byref(p),
            _ptr(idx_v_u), _ptr(a_K_r_m_rbar_v_s_u)), "rslf_kernel_columns_pile")
    return st


def compute_1D_depth_scores(vol: Volume, a_dmin_v_u, a_dmax_v_u, a_dim_d: int, a_s_hat: int,
                            parameters: Depth1DParameters | None = None, a_mask_v_u: torch.Tensor | None = None,
                            v_first: int = 0, n_rows: int | None = None, out: torch.Tensor | None = None, *,
                            want_stats: bool = False):
    """The scan's whole score matrix (core.hpp:616-625, the caller's BufferDepth1D::buf_scores_u_d) for the scanlines
    [v_first, v_first + n_rows) -> [n_rows, U, D] f32 on the volume's device, score[d] of every pixel whose byte of
    a_mask_v_u ([V,U] u8, read-only; None: every pixel) is set.  Rows of other pixels keep what `out` held (zeros when
    the tensor is made here).  a_dmin_v_u / a_dmax_v_u: [V,U] f32 CUDA tensors or Python floats.  To reproduce the
    reference pass the mask a scan was entered with (edge mask AND scan mask).  want_stats: returns (scores, rslf_stats)."""
    p = (parameters or Depth1DParameters()).to_c()
    planes = isinstance(a_dmin_v_u, torch.Tensor)
    n_rows = vol.V - int(v_first) if n_rows is None else int(n_rows)
    shape = (max(n_rows, 0), vol.U, int(a_dim_d))
    if out is None:
        out = torch.zeros(shape, dtype=torch.float32, device=vol.ctx.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 CUDA tensor of shape %s" % (shape,))
    if a_mask_v_u is not None and (tuple(a_mask_v_u.shape) != (vol.V, vol.U) or a_mask_v_u.dtype != torch.uint8
                                   or not a_mask_v_u.is_contiguous()):
        raise ValueError("a_mask_v_u must be a contiguous uint8 [V, U] plane")
    st = RslfStats() if want_stats else None
    vol.ctx.use_current_stream()
    check(_lib.lib().rslf_depth_epi_scores(
        vol.ctx._h, vol._h, _ptr(a_dmin_v_u if planes else None), _ptr(a_dmax_v_u if planes else None),
        0.0 if planes else float(a_dmin_v_u), 0.0 if planes else float(a_dmax_v_u), int(a_dim_d), int(a_s_hat), C.byref(p),
        _ptr(a_mask_v_u), int(v_first), n_rows, _ptr(out), C.byref(st) if st is not None else None), "rslf_depth_epi_scores")
    return (out, st) if want_stats else out


class Peaks(NamedTuple):
    """The peaks of score rows, [n_rows, U] each: the winner's index and score (the scan's arg max), the sub-grid
    disparity (the vertex of the parabola through the winner and its two neighbours, within half a grid step of the
    winner's grid value), and the runner-up peak's index (-1: none) and score (0 without one).  include/rslf_hip.h,
    rslf_peaks, states the arithmetic."""
    idx: Optional[torch.Tensor]
    score: Optional[torch.Tensor]
    disp: Optional[torch.Tensor]
    runner_idx: Optional[torch.Tensor]
    runner_score: Optional[torch.Tensor]


def _peak_planes(out: Peaks | None, n_rows: int, U: int, device) -> tuple[Peaks, _lib.RslfPeaks]:
    """The planes a peaks call writes -- made here (-1 / 0, what an unscanned pixel keeps) or the caller's, of which some
    may be None -- and the C struct of their pointers."""
    shape = (max(n_rows, 0), U)
    if out is None:
        out = Peaks(*(torch.full(shape, -1, dtype=torch.int32, device=device) if name.endswith("idx")
                      else torch.zeros(shape, dtype=torch.float32, device=device) for name in Peaks._fields))
    else:
        out = Peaks(*out)
        for name, t in zip(Peaks._fields, out):
            want = torch.int32 if name.endswith("idx") else torch.float32
            if t is not None and (tuple(t.shape) != shape or t.dtype != want or not t.is_cuda or not t.is_contiguous()):
                raise ValueError("out.%s must be a contiguous %s CUDA tensor of shape %s" % (name, want, shape))
    return out, _lib.RslfPeaks(*(None if t is None else t.data_ptr() for t in out))


def _sweep_peak_planes(out: "Peaks", S: int, V: int, U: int) -> _lib.RslfPeaks:
    """The C struct of a sweep's four peak planes [S, V, U] (rslf_sweep_peaks): members may be None, not all; disp must be."""
    out = Peaks(*out)
    if out.disp is not None:
        raise ValueError("peaks.disp must be None: the sub-grid mode puts that value in the depth plane")
    for name, t in zip(Peaks._fields, out):
        want = torch.int32 if name.endswith("idx") else torch.float32
        if t is not None and (tuple(t.shape) != (S, V, U) or t.dtype != want or not t.is_cuda or not t.is_contiguous()):
            raise ValueError("peaks.%s must be a contiguous %s CUDA tensor of shape %s" % (name, want, (S, V, U)))
    if all(t is None for t in out):
        raise ValueError("peaks: all four planes are None, nothing to compute")
    return _lib.RslfPeaks(*(None if t is None else t.data_ptr() for t in out))


def _check_mask_plane(a_mask_v_u, V: int | None, U: int) -> None:
    if a_mask_v_u is not None and (a_mask_v_u.dim() != 2 or a_mask_v_u.shape[1] != U or (V is not None and a_mask_v_u.shape[0] != V)
                                   or a_mask_v_u.dtype != torch.uint8 or not a_mask_v_u.is_contiguous()):
        raise ValueError("a_mask_v_u must be a contiguous uint8 [V, U] plane")


def score_peaks(scores: torch.Tensor, a_dmin_v_u, a_dmax_v_u, a_mask_v_u: torch.Tensor | None = None, v_first: int = 0,
                out: Peaks | None = None, ctx: Context | None = None) -> Peaks:
    """Peaks of score rows the caller holds: `scores` is [n_rows, U, D] f32 on the device, as compute_1D_depth_scores
    returns it for the scanlines from v_first on.  a_dmin_v_u / a_dmax_v_u: Python floats, or full [V, U] f32 planes read
    at those scanlines, like the mask ([V, U] u8; None: every pixel).  Pixels outside the mask keep what `out` held
    (-1 / 0 when the tensors are made here); members of `out` may be None, not all.  Nothing leaves the device."""
    if scores.dim() != 3 or scores.dtype != torch.float32 or not scores.is_cuda or not scores.is_contiguous():
        raise ValueError("scores must be a contiguous float32 CUDA tensor [n_rows, U, D]")
    n_rows, U, D = (int(x) for x in scores.shape)
    planes = isinstance(a_dmin_v_u, torch.Tensor)
    _check_mask_plane(a_mask_v_u, None, U)
    for t in ((a_mask_v_u, a_dmin_v_u, a_dmax_v_u) if planes else (a_mask_v_u,)):
        if t is not None and (t.dim() != 2 or t.shape[1] != U or t.shape[0] < int(v_first) + n_rows):
            raise ValueError("the mask and the range planes are [V, U] planes that hold the scanlines [v_first, v_first + n_rows)")
    ctx = ctx or default_context(scores.device)
    out, c_out = _peak_planes(out, n_rows, U, scores.device)
    ctx.use_current_stream()
    check(_lib.lib().rslf_score_peaks(
        ctx._h, _ptr(scores), U, D, _ptr(a_dmin_v_u if planes else None), _ptr(a_dmax_v_u if planes else None),
        0.0 if planes else float(a_dmin_v_u), 0.0 if planes else float(a_dmax_v_u), _ptr(a_mask_v_u), int(v_first), n_rows,
        C.byref(c_out)), "rslf_score_peaks")
    return out


def compute_1D_depth_peaks(vol: Volume, a_dmin_v_u, a_dmax_v_u, a_dim_d: int, a_s_hat: int,
                           parameters: Depth1DParameters | None = None, a_mask_v_u: torch.Tensor | None = None,
                           v_first: int = 0, n_rows: int | None = None, out: Peaks | None = None, *, want_stats: bool = False):
    """Score rows and their peaks for the scanlines [v_first, v_first + n_rows) -> Peaks of [n_rows, U] tensors on the
    volume's device.  Arguments as compute_1D_depth_scores; the rows themselves pass through the context's staging buffer
    and are not kept.  want_stats: returns (peaks, rslf_stats), and waits."""
    p = (parameters or Depth1DParameters()).to_c()
    planes = isinstance(a_dmin_v_u, torch.Tensor)
    n_rows = vol.V - int(v_first) if n_rows is None else int(n_rows)
    _check_mask_plane(a_mask_v_u, vol.V, vol.U)
    out, c_out = _peak_planes(out, n_rows, vol.U, vol.ctx.device)
    st = RslfStats() if want_stats else None
    vol.ctx.use_current_stream()
    check(_lib.lib().rslf_depth_epi_peaks(
        vol.ctx._h, vol._h, _ptr(a_dmin_v_u if planes else None), _ptr(a_dmax_v_u if planes else None),
        0.0 if planes else float(a_dmin_v_u), 0.0 if planes else float(a_dmax_v_u), int(a_dim_d), int(a_s_hat), C.byref(p),
        _ptr(a_mask_v_u), int(v_first), n_rows, C.byref(c_out), C.byref(st) if st is not None else None), "rslf_depth_epi_peaks")
    return (out, st) if want_stats else out


class SubGrid(NamedTuple):
    """What subgrid_refine writes, [V, U] f32 each: the sub-grid disparity (Peaks.disp, from three scores instead of a row)
    and the scores of the winner's two neighbours (0 at the end of the grid that has none)."""
    disp: torch.Tensor
    left: Optional[torch.Tensor]
    right: Optional[torch.Tensor]


def subgrid_refine(vol: Volume, a_dmin_v_u, a_dmax_v_u, a_dim_d: int, a_s_hat: int, idx_v_u: torch.Tensor,
                   score_v_u: torch.Tensor | None = None, parameters: Depth1DParameters | None = None, *,
                   disp: torch.Tensor | None = None, left: torch.Tensor | None = None, right: torch.Tensor | None = None,
                   neighbours: bool = True) -> SubGrid:
    """A scan's arg max moved off the hypothesis grid: for every pixel with idx >= 0 the hypotheses idx - 1 and idx + 1
    are scored again (and idx itself without score_v_u) and the parabola through the three scores gives `disp`, within
    half a grid step of the grid value.  idx_v_u / score_v_u: the planes a scan of the same volume, range, a_dim_d,
    a_s_hat and parameters wrote.  Pixels with idx < 0 keep what the output planes held (zeros when made here); `disp`
    may be the scan's depth plane.  neighbours=False: no left / right planes unless given.  No score row is made."""
    p = (parameters or Depth1DParameters()).to_c()
    planes = isinstance(a_dmin_v_u, torch.Tensor)
    shape = (vol.V, vol.U)
    if tuple(idx_v_u.shape) != shape or idx_v_u.dtype != torch.int32 or not idx_v_u.is_cuda or not idx_v_u.is_contiguous():
        raise ValueError("idx_v_u must be a contiguous int32 CUDA tensor of shape %s" % (shape,))
    if disp is None:
        disp = torch.zeros(shape, dtype=torch.float32, device=idx_v_u.device)
    if neighbours and left is None:
        left = torch.zeros(shape, dtype=torch.float32, device=idx_v_u.device)
    if neighbours and right is None:
        right = torch.zeros(shape, dtype=torch.float32, device=idx_v_u.device)
    for name, t in (("score_v_u", score_v_u), ("disp", disp), ("left", left), ("right", right)):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous()):
            raise ValueError("%s must be a contiguous float32 CUDA tensor of shape %s" % (name, shape))
    vol.ctx.use_current_stream()
    check(_lib.lib().rslf_subgrid_refine(
        vol.ctx._h, vol._h, _ptr(a_dmin_v_u if planes else None), _ptr(a_dmax_v_u if planes else None),
        0.0 if planes else float(a_dmin_v_u), 0.0 if planes else float(a_dmax_v_u), int(a_dim_d), int(a_s_hat), C.byref(p),
        _ptr(idx_v_u), _ptr(score_v_u), _ptr(disp), _ptr(left), _ptr(right)), "rslf_subgrid_refine")
    return SubGrid(disp, left, right)


def selective_median_filter(a_src: torch.Tensor, vol: Volume, a_s_hat: int, a_size: int, a_mask_v_u: torch.Tensor,
                            a_epsilon: float) -> torch.Tensor:
    """core.hpp:366-375; returns a_dst."""
    dst = torch.empty_like(a_src)
    vol.ctx.use_current_stream()
    check(_lib.lib().rslf_selective_median(vol.ctx._h, vol._h, _ptr(a_src), _ptr(dst), a_s_hat, a_size,
                                           _ptr(a_mask_v_u), float(a_epsilon)), "rslf_selective_median")
    return dst


# ---- the reference's class -------------------------------------------------

class Depth1DComputer_pile:
    """rslf::Depth1DComputer_pile<T> (dc.hpp:93-143).

    `epis` is the reference's Vec<Mat> (a list of V arrays [S,U] or [S,U,3],
    uint8 or float32), a dense numpy / CUDA array [V,S,U(,C)], or a Volume that
    is already resident.  After run(), the result members hold CUDA tensors."""

    def __init__(self, epis, dmin: float, dmax: float, dim_d: int, s_hat: int = -1, epi_scale_factor: float = -1.0,
                 parameters: Depth1DParameters | None = None, ctx: Context | None = None, subgrid: bool = False,
                 u_dilation: int = 1, dilation_kind=DILATE_CUBIC):
        self.m_parameters = parameters or Depth1DParameters.get_default()
        # not in the reference: the EPIs are dilated along u on the device (Volume.dilated_u) and the object behaves bit for
        # bit as if built from the dilated EPIs with par_slope_factor * u_dilation: every member is U' wide; undilated()
        # brings a plane back.  1: nothing happens
        self.m_u_dilation, self.m_dilation_kind = _u_dilation(u_dilation, dilation_kind, "Depth1DComputer_pile")
        # not in the reference: the scan's disparities are moved off the hypothesis grid before the median (subgrid_refine);
        # m_depth_raw_v_u is then the refined plane, and the getters show refined values
        self.m_subgrid = bool(subgrid)
        if isinstance(epis, Volume):
            self.m_epis = epis
        elif isinstance(epis, (list, tuple)):
            self.m_epis = Volume.from_epis(epis, epi_scale_factor, ctx)
        elif isinstance(epis, np.ndarray):
            a = epis[..., 0] if (epis.ndim == 4 and epis.shape[3] == 1) else epis
            self.m_epis = Volume.from_epis(list(a), epi_scale_factor, ctx)
        else:
            self.m_epis = Volume.from_dense(epis, epi_scale_factor if epi_scale_factor > 0 else 1.0, ctx)
        if self.m_u_dilation != 1:
            self.m_epis = self.m_epis.dilated_u(self.m_u_dilation, self.m_dilation_kind)
            self.m_parameters = _dilated_parameters(self.m_parameters, self.m_u_dilation)
        vol = self.m_epis
        self.m_dim_d = int(dim_d)
        self.m_dmin, self.m_dmax = float(dmin), float(dmax)
        # dc.hpp:490-498
        self.m_s_hat = int(np.floor((0.0 + vol.S) / 2)) if (s_hat < 0 or s_hat > vol.S - 1) else int(s_hat)
        dev = vol.ctx.device
        V, U, C_ = vol.V, vol.U, vol.C
        self.m_edge_confidence_v_u = torch.empty((V, U), dtype=torch.float32, device=dev)
        self.m_edge_confidence_mask_v_u = torch.empty((V, U), dtype=torch.uint8, device=dev)
        self.m_disp_confidence_v_u = torch.empty((V, U), dtype=torch.float32, device=dev)
        self.m_best_depth_v_u = torch.empty((V, U), dtype=torch.float32, device=dev)
        self.m_rbar_v_u = torch.empty((V, U, C_), dtype=torch.float32, device=dev)
        # parity witnesses, not in the reference
        self.m_depth_idx_v_u = torch.empty((V, U), dtype=torch.int32, device=dev)
        self.m_score_v_u = torch.empty((V, U), dtype=torch.float32, device=dev)
        self.m_depth_raw_v_u = torch.empty((V, U), dtype=torch.float32, device=dev)
        self.stats: RslfStats | None = None

    def run(self, want_stats: bool = True) -> None:
        """dc.hpp:513-565."""
        vol = self.m_epis
        p = self.m_parameters.to_c()
        st = RslfStats() if want_stats else None
        vol.ctx.use_current_stream()
        args = (vol.ctx._h, vol._h, self.m_dmin, self.m_dmax, self.m_dim_d, self.m_s_hat, C.byref(p),
                _ptr(self.m_edge_confidence_v_u), _ptr(self.m_edge_confidence_mask_v_u), _ptr(self.m_disp_confidence_v_u),
                _ptr(self.m_best_depth_v_u), _ptr(self.m_rbar_v_u), _ptr(self.m_depth_idx_v_u), _ptr(self.m_score_v_u),
                _ptr(self.m_depth_raw_v_u), C.byref(st) if st is not None else None)
        if self.m_subgrid:
            check(_lib.lib().rslf_depth1d_pile_run_sub(*args, 1), "rslf_depth1d_pile_run_sub")
        else:
            check(_lib.lib().rslf_depth1d_pile_run(*args), "rslf_depth1d_pile_run")
        self.stats = st
        self._ran = True

    def get_s_hat(self) -> int:
        return self.m_s_hat

    def undilated(self, name: str) -> torch.Tensor:
        """A result plane on the source grid, [V, U] (rbar [V, U, C]): its columns u * u_dilation.  Names: depth, valid
        (the edge mask), edge_confidence, disp_confidence, rbar, depth_idx, score, depth_raw.  With u_dilation = 1 the
        member itself."""
        planes = dict(depth=self.m_best_depth_v_u, valid=self.m_edge_confidence_mask_v_u, edge_confidence=self.m_edge_confidence_v_u,
                      disp_confidence=self.m_disp_confidence_v_u, rbar=self.m_rbar_v_u, depth_idx=self.m_depth_idx_v_u,
                      score=self.m_score_v_u, depth_raw=self.m_depth_raw_v_u)
        return _undilated("Depth1DComputer_pile", planes, name, self.m_epis, ("rbar",))

    def get_coloured_epi(self, a_v=-1, lut_bgr=None) -> torch.Tensor:
        """dc.hpp:568-617: the EPI of scanline a_v (< 0: floor(V / 2.0)) with every confident pixel's line drawn in the
        colour of its disparity, nearer lines over farther ones -> [S, U, 3] uint8 BGR on the device.  a_v may be a
        range: [len, S, U, 3] in one call.  lut_bgr ([256, 3] uint8) stands where the reference takes a_cv_colormap (None:
        colormap_jet()).  The reference's loop races under OpenMP; this is its sequential meaning (a target keeps the
        greatest depth, of equal depths the smallest u).  A NaN depth draws nothing."""
        vol = self.m_epis
        return _coloured_epi_rows(vol.ctx, self.m_best_depth_v_u, self.m_edge_confidence_mask_v_u, vol.S, self.m_s_hat, a_v, lut_bgr)

    def get_disparity_map(self, lut_bgr=None) -> torch.Tensor:
        """dc.hpp:619-643: the disparities scaled over their min / max (every pixel, confident or not), colour-mapped,
        black outside m_edge_confidence_mask_v_u -> [V, U, 3] uint8 BGR.  What a NaN disparity gives is unspecified."""
        ctx = self.m_epis.ctx
        lo, hi = render_fit(ctx, self.m_best_depth_v_u, None, FIT_MINMAX)
        return render_planes(ctx, self.m_best_depth_v_u.unsqueeze(0), lo, hi, RENDER_SHIFT, lut_bgr,
                             self.m_edge_confidence_mask_v_u.unsqueeze(0), MASK_BLACK)[0]

    def get_scores(self, v_first: int = 0, n_rows: int | None = None) -> torch.Tensor:
        """After run(): the score rows [n_rows, U, D] of scanlines [v_first, v_first + n_rows), the reference's
        buf_scores_u_d of each EPI (core.hpp:616-625), over the pixels of the FINAL edge-confidence mask -- those that
        received a disparity; the rows of every other pixel are 0.  (The reference also fills the rows of pixels it then
        rejects at raw_score_threshold; to get those, call compute_1D_depth_scores with the mask the scan was entered
        with.)  A scan of its own: the scores are computed again, nothing is kept from run()."""
        if not getattr(self, "_ran", False):
            raise RuntimeError("get_scores shows the pixels run() gave a disparity: call run() first")
        return compute_1D_depth_scores(self.m_epis, self.m_dmin, self.m_dmax, self.m_dim_d, self.m_s_hat, self.m_parameters,
                                       self.m_edge_confidence_mask_v_u, v_first, n_rows)

    def get_peaks(self, v_first: int = 0, n_rows: int | None = None) -> Peaks:
        """After run(): the peaks of the score rows of scanlines [v_first, v_first + n_rows) over the pixels of the final
        edge-confidence mask, like get_scores -> Peaks of [n_rows, U] tensors: idx equals m_depth_idx_v_u and score
        m_score_v_u there, disp is the winner's grid value moved by at most half a grid step, runner_idx / runner_score the
        second peak.  Other pixels hold -1 / 0.  A scan of its own; the rows stay on the device and are not kept."""
        if not getattr(self, "_ran", False):
            raise RuntimeError("get_peaks shows the pixels run() gave a disparity: call run() first")
        return compute_1D_depth_peaks(self.m_epis, self.m_dmin, self.m_dmax, self.m_dim_d, self.m_s_hat, self.m_parameters,
                                      self.m_edge_confidence_mask_v_u, v_first, n_rows)

    def results(self) -> dict:
        """Host copies of every output plane."""
        torch.cuda.synchronize(self.m_epis.ctx.device)
        return dict(
            edge_confidence=self.m_edge_confidence_v_u.cpu().numpy(),
            edge_mask=self.m_edge_confidence_mask_v_u.cpu().numpy(),
            disp_confidence=self.m_disp_confidence_v_u.cpu().numpy(),
            depth=self.m_best_depth_v_u.cpu().numpy(),
            rbar=self.m_rbar_v_u.cpu().numpy(),
            depth_idx=self.m_depth_idx_v_u.cpu().numpy(),
            score=self.m_score_v_u.cpu().numpy(),
            depth_raw=self.m_depth_raw_v_u.cpu().numpy(),
        )


def host_rows(arrays: Sequence[np.ndarray], dtype, in_place: bool = True):
    """Host arrays of one shape ([rows, U] or [rows, U, C]: EPIs or images) as the C-ABI's host-pointer entries take them:
    (the arrays, to be kept alive over the call; their pointers; row_stride_bytes).  Rows with padding between them -- a window
    `parent[:, a:b]` of a wider array, the reference's ROI Mat with its cv::Mat::step -- go up where they lie: an array is
    taken in place when it is a numpy.ndarray of `dtype` whose rows are dense (the strides of a C-contiguous [U] / [U, C]
    row) and lie a positive stride of at least one row apart.  When every array is, and all share that stride, it is the
    row_stride_bytes; otherwise every array goes as a dense copy (an array that is dense already as it is) and the stride is
    0, as it is for a list of dense arrays.  `in_place=False`: always the dense form."""
    dt = np.dtype(dtype)

    def stride_in_place(a) -> int:
        """The row stride `a` can be read with where it lies, or -1."""
        if not isinstance(a, np.ndarray) or a.dtype != dt or a.ndim not in (2, 3):
            return -1
        row_bytes, inner = dt.itemsize, a.ndim - 1
        for k in range(inner, 0, -1):          # dense within a row (an axis of one element has no stride to speak of)
            if a.shape[k] != 1 and a.strides[k] != row_bytes:
                return -1
            row_bytes *= a.shape[k]
        if a.shape[0] == 1:
            return row_bytes
        return a.strides[0] if a.strides[0] >= row_bytes else -1

    # a thousand EPIs: no per-array conversions or ctypes objects where none are needed
    strides = [stride_in_place(a) for a in arrays] if in_place else []
    if strides and strides[0] > 0 and all(st == strides[0] for st in strides):
        keep, stride = list(arrays), strides[0]
    else:
        keep = [a if (type(a) is np.ndarray and a.dtype == dt and a.flags.c_contiguous) else np.ascontiguousarray(a, dtype=dt)
                for a in arrays]
        stride = 0
    if any(a.shape != keep[0].shape for a in keep):
        raise ValueError("every array must have the shape of the first, %s" % (keep[0].shape,))
    if stride and stride == int(np.prod(keep[0].shape[1:])) * dt.itemsize:
        stride = 0                             # dense rows
    ptrs = (C.c_void_p * len(keep))(*[a.__array_interface__["data"][0] for a in keep])
    return keep, ptrs, stride


def host_epis(epis: Sequence[np.ndarray], dtype=None, stride: bool = False):
    """A host EPI list (the reference's Vec<Mat>: V arrays [S,U] or [S,U,3]) as the C-ABI takes it: (the arrays, to be
    kept alive over the call; their pointers; their element type; V, S, U, C).  Every EPI goes as `dtype`, by default
    the first one's, and must have the first one's shape.  With `stride=True` the row_stride_bytes to pass is returned as an
    eighth value and padded rows go up in place (host_rows); without it every EPI is dense, for callers that pass stride 0."""
    dt = np.asarray(epis[0]).dtype if dtype is None else np.dtype(dtype)
    if dt not in (np.uint8, np.uint16, np.float32):
        raise TypeError("EPIs must be uint8, uint16 or float32 (dc.hpp:149-154)")
    keep, ptrs, row_stride = host_rows(epis, dt, in_place=stride)
    S, U = keep[0].shape[0], keep[0].shape[1]
    C_ = 1 if keep[0].ndim == 2 else keep[0].shape[2]
    out = (keep, ptrs, dt, len(keep), S, U, C_)
    return out + (row_stride,) if stride else out


class MultiDevice:
    """rslf_multi: Depth1DComputer_pile's constructor + run() + result Mats in one call on HOST arrays, the scanlines cut
    into one block per device (and every block into chunks whose upload, kernels and download overlap).  Host planes
    come back as numpy arrays; no collective is involved (each device writes its rows of the caller's planes)."""

    def __init__(self, devices: Sequence[int] | None = None):
        devs = list(devices) if devices else []
        arr = (C.c_int * max(1, len(devs)))(*devs) if devs else None
        h = C.c_void_p()
        check(_lib.lib().rslf_multi_create(arr, len(devs), C.byref(h)), "rslf_multi_create")
        self._h = h

    def device_count(self) -> int:
        return int(_lib.lib().rslf_multi_device_count(self._h))

    def set_chunk_rows(self, rows: int) -> None:
        check(_lib.lib().rslf_multi_set_chunk_rows(self._h, int(rows)), "rslf_multi_set_chunk_rows")

    def peer_access(self) -> list:
        """n x n matrix: [i][k] = 1 if worker i reaches worker k's memory directly (same GPU, or peer access enabled over
        xGMI), 0 if copies between them stage through the host (rslf_multi_peer_access)."""
        n = self.device_count()
        return [[int(_lib.lib().rslf_multi_peer_access(self._h, i, k)) for k in range(n)] for i in range(n)]

    def depth1d_pile(self, epis: Sequence[np.ndarray], dmin: float, dmax: float, dim_d: int, s_hat: int = -1,
                     epi_scale_factor: float = -1.0, parameters: Depth1DParameters | None = None, subgrid: bool = False,
                     u_dilation: int = 1) -> dict:
        """epis: the reference's Vec<Mat> -- V arrays [S,U] or [S,U,3], all uint8, all uint16 or all float32."""
        require_no_subgrid(subgrid, "MultiDevice.depth1d_pile")
        require_no_u_dilation(u_dilation, "MultiDevice.depth1d_pile")
        keep, ptrs, dt, V, S, U, C_, stride = host_epis(epis, stride=True)
        out = dict(edge_confidence=np.empty((V, U), np.float32), edge_mask=np.empty((V, U), np.uint8),
                   disp_confidence=np.empty((V, U), np.float32), depth=np.empty((V, U), np.float32),
                   rbar=np.empty((V, U, C_), np.float32), depth_idx=np.empty((V, U), np.int32),
                   score=np.empty((V, U), np.float32), depth_raw=np.empty((V, U), np.float32))
        hp = [out[k].ctypes.data_as(C.c_void_p) for k in ("edge_confidence", "edge_mask", "disp_confidence", "depth", "rbar",
                                                         "depth_idx", "score", "depth_raw")]
        p = (parameters or Depth1DParameters()).to_c()
        st = RslfStats()
        L = _lib.lib()
        if dt == np.uint8:
            check(L.rslf_multi_depth1d_pile_u8(self._h, ptrs, stride, V, S, U, C_, float(dmin), float(dmax), int(dim_d), int(s_hat),
                                               C.byref(p), *hp, C.byref(st)), "rslf_multi_depth1d_pile_u8")
            self.scale_used = 255.0
        else:
            su = C.c_float()
            name = "rslf_multi_depth1d_pile_" + _SUFFIX[dt]
            check(getattr(L, name)(self._h, ptrs, stride, V, S, U, C_, float(epi_scale_factor), float(dmin), float(dmax),
                                   int(dim_d), int(s_hat), C.byref(p), *hp, C.byref(st), C.byref(su)), name)
            self.scale_used = float(su.value)
        self.stats = st
        return out

    def depth2d(self, epis: Sequence[np.ndarray], dmin: float, dmax: float, dim_d: int, epi_scale_factor: float = -1.0,
                parameters: Depth1DParameters | None = None, subgrid: bool = False, peaks=None, propagation_ratio=None,
                u_dilation: int = 1) -> dict:
        """Depth2DComputer (constructor + run + getters) over this object's devices: the 2-D sweep cut into one block of
        scanlines per device, the neighbours' boundary rows exchanged by peer copy on every visit
        (rslf_multi_depth2d_run_f32 / _u8 / _u16).  Host EPIs in, numpy planes [S, V, U] out."""
        require_no_subgrid(subgrid, "MultiDevice.depth2d")
        require_no_peaks(peaks, "MultiDevice.depth2d")
        require_no_propagation_ratio(propagation_ratio, "MultiDevice.depth2d")
        require_no_u_dilation(u_dilation, "MultiDevice.depth2d")
        keep, ptrs, dt, V, S, U, C_, stride = host_epis(epis, stride=True)
        out = dict(edge_confidence=np.empty((S, V, U), np.float32), edge_mask=np.empty((S, V, U), np.uint8),
                   disp_confidence=np.empty((S, V, U), np.float32), depth=np.empty((S, V, U), np.float32),
                   rbar=np.empty((S, V, U, C_), np.float32), scan_mask=np.empty((S, V, U), np.uint8))
        hp = [out[k].ctypes.data_as(C.c_void_p) for k in ("edge_confidence", "edge_mask", "disp_confidence", "depth", "rbar", "scan_mask")]
        require_no_line_confidence(parameters, "MultiDevice.depth2d")
        p = (parameters or Depth1DParameters()).to_c()
        st = RslfStats()
        L = _lib.lib()
        if dt == np.uint8:
            check(L.rslf_multi_depth2d_run_u8(self._h, ptrs, stride, V, S, U, C_, float(dmin), float(dmax), int(dim_d), C.byref(p), *hp,
                                              C.byref(st)), "rslf_multi_depth2d_run_u8")
            self.scale_used = 255.0
        else:
            su = C.c_float()
            name = "rslf_multi_depth2d_run_" + _SUFFIX[dt]
            check(getattr(L, name)(self._h, ptrs, stride, V, S, U, C_, float(epi_scale_factor), float(dmin), float(dmax),
                                   int(dim_d), C.byref(p), *hp, C.byref(st), C.byref(su)), name)
            self.scale_used = float(su.value)
        self.stats = st
        return out

    def fine_to_coarse(self, epis: Sequence[np.ndarray], d_min: float, d_max: float, dim_d: int, epi_scale_factor: float = -1.0,
                       parameters: Depth1DParameters | None = None, max_pyr_depth: int = -1, accept_all_last_scale: bool = True,
                       subgrid: bool = False, peaks=None, propagation_ratio=None, consistency_min_agree=None, u_dilation: int = 1,
                       *, equalize_views=None, level_dilation: int = 1, derivative_channels: float = 0.0):
        """FineToCoarse (constructor + run + get_results) over this object's devices (rslf_multi_fine_to_coarse_run_host):
        every level's sweep sharded by scanline.  Returns (out_map [S,V,U] f32, out_validity [S,V,U] u8, levels)."""
        require_no_subgrid(subgrid, "MultiDevice.fine_to_coarse")
        require_no_peaks(peaks, "MultiDevice.fine_to_coarse")
        require_no_propagation_ratio(propagation_ratio, "MultiDevice.fine_to_coarse")
        require_no_consistency_gate(consistency_min_agree, "MultiDevice.fine_to_coarse")
        require_no_u_dilation(u_dilation, "MultiDevice.fine_to_coarse")
        require_no_derivative_channels(derivative_channels, "MultiDevice.fine_to_coarse")
        require_no_equalize_views(equalize_views, "MultiDevice.fine_to_coarse")
        require_no_level_dilation(level_dilation, "MultiDevice.fine_to_coarse")
        keep, ptrs, dt, V, S, U, C_, stride = host_epis(epis, stride=True)
        out_map = np.empty((S, V, U), np.float32)
        out_valid = np.empty((S, V, U), np.uint8)
        require_no_line_confidence(parameters, "MultiDevice.fine_to_coarse")
        p = (parameters or Depth1DParameters()).to_c()
        st, nl = RslfStats(), C.c_int()
        rest = (V, S, U, C_, stride, float(d_min), float(d_max), int(dim_d), float(epi_scale_factor), C.byref(p), int(max_pyr_depth),
                1 if accept_all_last_scale else 0, out_map.ctypes.data_as(C.c_void_p), out_valid.ctypes.data_as(C.c_void_p),
                C.byref(nl), C.byref(st))
        if dt == np.uint16:   # ushort arithmetic through the pyramid
            check(_lib.lib().rslf_multi_fine_to_coarse_run_host_u16(self._h, ptrs, *rest), "rslf_multi_fine_to_coarse_run_host_u16")
        else:
            check(_lib.lib().rslf_multi_fine_to_coarse_run_host(self._h, ptrs, 1 if dt == np.uint8 else 0, *rest),
                  "rslf_multi_fine_to_coarse_run_host")
        self.stats = st
        return out_map, out_valid, int(nl.value)

    def get_consistency(self, *args, **kwargs):
        no_consistency("MultiDevice")

    def get_warped_views(self, *args, **kwargs):
        no_view_warp("MultiDevice")

    def get_view_prediction(self, *args, **kwargs):
        no_view_warp("MultiDevice", "get_view_prediction")

    def get_novel_views(self, *args, **kwargs):
        no_novel_view("MultiDevice")

    def get_novel_view_prediction(self, *args, **kwargs):
        no_novel_view("MultiDevice", "get_novel_view_prediction")

    def depth1d_pile_device_out(self, epis: Sequence[np.ndarray], dmin: float, dmax: float, dim_d: int, out_device: int = 0,
                                s_hat: int = -1, epi_scale_factor: float = -1.0, parameters: Depth1DParameters | None = None,
                                subgrid: bool = False, u_dilation: int = 1) -> dict:
        """The same with the result planes left on `out_device` as CUDA tensors (float32 EPIs): every worker copies its
        rows there with a peer copy (rslf_multi_depth1d_pile_f32_dev)."""
        require_no_subgrid(subgrid, "MultiDevice.depth1d_pile_device_out")
        require_no_u_dilation(u_dilation, "MultiDevice.depth1d_pile_device_out")
        keep, ptrs, _, V, S, U, C_, stride = host_epis(epis, np.float32, stride=True)
        dev = torch.device("cuda", out_device)
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        out = dict(edge_confidence=mk((V, U), torch.float32), edge_mask=mk((V, U), torch.uint8), disp_confidence=mk((V, U), torch.float32),
                   depth=mk((V, U), torch.float32), rbar=mk((V, U, C_), torch.float32), depth_idx=mk((V, U), torch.int32),
                   score=mk((V, U), torch.float32), depth_raw=mk((V, U), torch.float32))
        torch.cuda.synchronize(dev)
        hp = [_ptr(out[k]) for k in ("edge_confidence", "edge_mask", "disp_confidence", "depth", "rbar", "depth_idx", "score", "depth_raw")]
        p = (parameters or Depth1DParameters()).to_c()
        st, su = RslfStats(), C.c_float()
        check(_lib.lib().rslf_multi_depth1d_pile_f32_dev(self._h, ptrs, stride, V, S, U, C_, float(epi_scale_factor), float(dmin), float(dmax),
                                                         int(dim_d), int(s_hat), C.byref(p), int(out_device), *hp, C.byref(st), C.byref(su)),
              "rslf_multi_depth1d_pile_f32_dev")
        self.stats, self.scale_used = st, float(su.value)
        return out

    def close(self) -> None:
        if getattr(self, "_h", None) and not sys.is_finalizing():
            _lib.lib().rslf_multi_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


# ---- "next" row: the 2-D sweep -------------------------

def compute_2D_edge_confidence(vol: Volume, a_edge_confidence_s_v_u: torch.Tensor,
                               a_parameters: Depth1DParameters | None = None) -> torch.Tensor:
    """core.hpp:323-330.  Accumulates into a_edge_confidence_s_v_u ([S,V,U] f32, pass zeros);
    returns the masks [S,V,U] u8."""
    p = (a_parameters or Depth1DParameters()).to_c()
    mask = torch.empty((vol.S, vol.V, vol.U), dtype=torch.uint8, device=a_edge_confidence_s_v_u.device)
    vol.ctx.use_current_stream()
    check(_lib.lib().rslf_edge_confidence_2d(vol.ctx._h, vol._h, C.byref(p), _ptr(a_edge_confidence_s_v_u), _ptr(mask)),
          "rslf_edge_confidence_2d")
    return mask


def line_confidence_pile(ctx: Context, a_s_hat: int, a_edge_confidence_s_v_u: torch.Tensor, a_K_r_m_rbar_v_s_u: torch.Tensor,
                         a_best_depth_v_u: torch.Tensor, a_edge_confidence_mask_v_u: torch.Tensor,
                         a_line_confidence_v_u: torch.Tensor) -> None:
    """core.hpp:1054-1079 for one visited view on caller planes: C_l = sum_s E K / sum_s K with E the edge confidence
    [S,V,U] interpolated along each pixel's line (slope a_best_depth_v_u [V,U], no slope factor) and K [V,S,U]; written
    into a_line_confidence_v_u [V,U] where a_edge_confidence_mask_v_u is set, left alone elsewhere."""
    S, V, U = a_edge_confidence_s_v_u.shape
    if tuple(a_K_r_m_rbar_v_s_u.shape) != (V, S, U) or tuple(a_best_depth_v_u.shape) != (V, U) \
            or tuple(a_edge_confidence_mask_v_u.shape) != (V, U) or tuple(a_line_confidence_v_u.shape) != (V, U):
        raise ValueError("line_confidence_pile: C_e is [S,V,U], K [V,S,U], the other planes [V,U]")
    ctx.use_current_stream()
    check(_lib.lib().rslf_line_confidence_pile(ctx._h, V, S, U, int(a_s_hat), _ptr(a_edge_confidence_s_v_u), _ptr(a_K_r_m_rbar_v_s_u),
                                               _ptr(a_best_depth_v_u), _ptr(a_edge_confidence_mask_v_u), _ptr(a_line_confidence_v_u)),
          "rslf_line_confidence_pile")


def compute_2D_depth_epi(vol: Volume, a_dmin_s_v_u, a_dmax_s_v_u, a_dim_d: int, a_edge_confidence_s_v_u: torch.Tensor,
                         a_edge_confidence_mask_s_v_u: torch.Tensor, a_disp_confidence_s_v_u: torch.Tensor,
                         a_best_depth_s_v_u: torch.Tensor, a_rbar_s_v_u: torch.Tensor,
                         a_parameters: Depth1DParameters | None = None, *, scan_mask_s_v_u: torch.Tensor | None = None,
                         want_stats: bool = False, a_line_confidence_s_v_u: torch.Tensor | None = None,
                         subgrid: bool = False, peaks: "Peaks | None" = None,
                         propagation_ratio: float | None = None) -> RslfStats | None:
    """core.hpp:336-351.  a_line_confidence_s_v_u ([S,V,U] f32, pass zeros) is the argument of the
    _USE_LINE_CONFIDENCE_SCORE build (:345): with it the call goes through rslf_depth_epi_2d_lc in
    a_parameters.par_line_confidence_mode -- mode 0 is then the default build and leaves the plane untouched; modes 1 and 2
    need the plane (without it the library returns RSLF_ERR_INVALID_ARG).
    a_dmin_s_v_u / a_dmax_s_v_u: [S,V,U] f32 CUDA tensors or Python floats.
    subgrid (not in the reference): every visit moves the disparities its scan wrote off the hypothesis grid before the
    median and the propagation read them (rslf_depth_epi_2d_sub).
    peaks (not in the reference): a Peaks of [S,V,U] planes (idx / runner_idx int32, score / runner_score f32, disp None;
    members may be None) -- every pixel a visit scans and accepts gets the winner and the runner-up peak of its score row,
    every pixel a visit paints its source's; the others keep what the planes held (rslf_depth_epi_2d_pk).  a_dim_d above
    2 ** 24 is refused.  Where the later visits still scan a large share of a view, Context.set_debug(peaks_list=0) is the
    faster form (include/rslf_hip.h, rslf_sweep_peaks).
    propagation_ratio (not in the reference; None or 0: off; else r in (0, 1], needs `peaks` with all four planes): a pixel
    whose runner-up scores more than r times its winner is withheld from propagation -- it makes no claim, keeps its raw
    disparity and stays in the running mask (rslf_depth_epi_2d_pr; the rule: include/rslf_hip.h,
    rslf_sweep_propagation_ratio).  Context.get_withheld_sources() then tells how many sources the sweep withheld."""
    ratio = _propagation_ratio(propagation_ratio, "compute_2D_depth_epi")
    if ratio and (peaks is None or any(getattr(peaks, k) is None for k in ("idx", "score", "runner_idx", "runner_score"))):
        raise ValueError("compute_2D_depth_epi: propagation_ratio reads the peak planes: pass peaks= with all four planes")
    par = a_parameters or Depth1DParameters()
    p = par.to_c()
    planes = isinstance(a_dmin_s_v_u, torch.Tensor)
    st = RslfStats() if want_stats else None
    vol.ctx.use_current_stream()
    args = (vol.ctx._h, vol._h, _ptr(a_dmin_s_v_u if planes else None), _ptr(a_dmax_s_v_u if planes else None),
            0.0 if planes else float(a_dmin_s_v_u), 0.0 if planes else float(a_dmax_s_v_u), a_dim_d,
            _ptr(a_edge_confidence_s_v_u), _ptr(a_edge_confidence_mask_s_v_u), _ptr(a_disp_confidence_s_v_u),
            _ptr(a_best_depth_s_v_u), _ptr(a_rbar_s_v_u), C.byref(p), _ptr(scan_mask_s_v_u),
            C.byref(st) if st is not None else None)
    mode = int(par.par_line_confidence_mode)
    c_pk = None if peaks is None else C.byref(_sweep_peak_planes(peaks, vol.S, vol.V, vol.U))
    # the family's widest entry: a mode that is off goes in neutral, and the call is the narrower entry's
    check(_lib.lib().rslf_depth_epi_2d_pr(*args, mode, _ptr(a_line_confidence_s_v_u), 1 if subgrid else 0, c_pk, ratio),
          "rslf_depth_epi_2d_pr")
    return st


class Consistency(NamedTuple):
    """Cross-view consistency of a sweep's disparity planes, [S, V, U] each (include/rslf_hip.h, rslf_view_consistency, states
    the rule): per pixel the other views that are in field (seen) and, of those, the ones whose pixel on the pixel's EPI line
    is valid and within tol (agree), more than tol above, more than tol below; fused, the mean of the pixel's disparity and
    the agreeing ones; valid, 255 where agree >= min_agree.  What above and below mean depends on the field's sign
    convention: with disparities that grow towards the camera, above is a legitimate occluder and below a free-space
    violation."""
    seen: Optional[torch.Tensor]
    agree: Optional[torch.Tensor]
    above: Optional[torch.Tensor]
    below: Optional[torch.Tensor]
    fused: Optional[torch.Tensor]
    valid: Optional[torch.Tensor]


def _consistency_args(tol, radius, min_agree, who: str) -> tuple[float, int, int]:
    tol = float(tol)
    if not 0.0 <= tol <= float(np.finfo(np.float32).max):   # (a NaN compares false; finite as the float32 it is sent as)
        raise ValueError("%s: tol %r is not a finite tolerance >= 0" % (who, tol))
    if int(min_agree) < 0:
        raise ValueError("%s: min_agree %r is negative" % (who, min_agree))
    return tol, int(radius), int(min_agree)


def _stack_tensors(who: str, depth_s_v_u: torch.Tensor, valid_s_v_u: torch.Tensor | None) -> tuple[int, int, int]:
    """The input planes of a stack operation (view_consistency, view_warp, novel_view), checked -> (S, V, U)."""
    if depth_s_v_u.dim() != 3 or depth_s_v_u.dtype != torch.float32 or not depth_s_v_u.is_cuda or not depth_s_v_u.is_contiguous():
        raise ValueError("%s: depth_s_v_u must be a contiguous float32 CUDA tensor [S, V, U]" % who)
    if valid_s_v_u is not None and (valid_s_v_u.shape != depth_s_v_u.shape or valid_s_v_u.dtype != torch.uint8
                                    or not valid_s_v_u.is_cuda or not valid_s_v_u.is_contiguous()):
        raise ValueError("%s: valid_s_v_u must be a contiguous uint8 CUDA tensor of depth_s_v_u's shape" % who)
    S, V, U = (int(x) for x in depth_s_v_u.shape)
    return S, V, U


def _consistency_out(shape, device, counts: bool, fused: bool) -> tuple[Consistency, _lib.RslfViewCounts]:
    """The planes a consistency call writes (seen .. below with counts, fused with fused, valid always) and the C struct."""
    new = lambda dtype: torch.empty(shape, dtype=dtype, device=device)
    cs = [new(torch.int32) if counts else None for _ in range(4)]
    out = Consistency(*cs, new(torch.float32) if fused else None, new(torch.uint8))
    return out, _lib.RslfViewCounts(*(None if t is None else t.data_ptr() for t in cs))


def view_consistency(ctx: Context, depth_s_v_u: torch.Tensor, valid_s_v_u: torch.Tensor | None, slope: float, tol: float,
                     radius: int = 0, min_agree: int = 0, counts: bool = True, fused: bool = True) -> Consistency:
    """rslf_view_consistency (not in the reference): do the views of a finished sweep agree with one another?  depth_s_v_u
    [S, V, U] f32 and valid_s_v_u ([S, V, U] u8, or None for every pixel) on the context's device; slope: the sweep's
    par_slope_factor; radius <= 0: every view, else only views within it.  Returns a Consistency of new tensors -- the four
    counts are None with counts=False, fused with fused=False.  Queued on the context's stream, not awaited."""
    tol, radius, min_agree = _consistency_args(tol, radius, min_agree, "view_consistency")
    S, V, U = _stack_tensors("view_consistency", depth_s_v_u, valid_s_v_u)
    out, c_counts = _consistency_out((S, V, U), depth_s_v_u.device, counts, fused)
    ctx.use_current_stream()
    check(_lib.lib().rslf_view_consistency(ctx._h, _ptr(depth_s_v_u), _ptr(valid_s_v_u), S, V, U, float(slope), tol, radius, min_agree,
                                           C.byref(c_counts), _ptr(out.fused), _ptr(out.valid)), "rslf_view_consistency")
    return out


def no_consistency(who: str) -> None:
    """The forms that have no consistency getter say so (no multi-device form before a multi-GPU lease)."""
    raise ValueError("%s: get_consistency is not built here: bring the [S, V, U] planes to one device and call view_consistency, "
                     "or use Depth2DComputer / fine_to_coarse_run_host(keep=True)" % who)


class Warp(NamedTuple):
    """The view warp's planes (include/rslf_hip.h, rslf_view_warp, states the rule), per target k of the T targets of a call;
    None where not asked for.  hit [T, V, U] uint8: 255 where a candidate arrived; depth f32: the winner's stored disparity
    (0 where none); src_view / src_col int32: the winner's view and column (-1 where none); count int32: the candidates that
    arrived; colour [T, V, U, C] f32: the volume's radiance at the winner (0 where none); err f32: the leave-one-out residual
    against the view that was taken; row_err [T, V] f64 / row_hits [T, V] int32: the sum of err over a row's hit pixels and
    their number."""
    hit: Optional[torch.Tensor]
    depth: Optional[torch.Tensor]
    src_view: Optional[torch.Tensor]
    src_col: Optional[torch.Tensor]
    count: Optional[torch.Tensor]
    colour: Optional[torch.Tensor]
    err: Optional[torch.Tensor]
    row_err: Optional[torch.Tensor]
    row_hits: Optional[torch.Tensor]


class ViewPrediction(NamedTuple):
    """The leave-one-out yardstick: err / hit [T, V, U] on the device (Warp's planes), and per target, as numpy float64 [T],
    mean_abs_error = row_err.sum() / row_hits.sum() (NaN where nothing arrived) and coverage = hits / (V * U)."""
    err: torch.Tensor
    hit: torch.Tensor
    mean_abs_error: np.ndarray
    coverage: np.ndarray
    row_err: torch.Tensor
    row_hits: torch.Tensor


WARP_MAX_TARGET = 65536.0   # kWarpMaxTarget (csrc/k14_warp_rule.hpp)


def _warp_args(targets, exclude, radius, nearer, who: str):
    """-> (c_float array, c_int array or None, T, radius, nearer); the refusals the library would make, made by name first."""
    targets = [float(t) for t in (targets.tolist() if hasattr(targets, "tolist") else targets)]
    if not targets:
        raise ValueError("%s: no targets" % who)
    for k, t in enumerate(targets):
        if not abs(t) <= WARP_MAX_TARGET:   # (a NaN compares false)
            raise ValueError("%s: targets[%d] = %r is not a finite position within +-65536" % (who, k, t))
    if int(nearer) == 0:
        raise ValueError("%s: nearer is +1 (larger disparities are nearer) or -1, not 0" % who)
    c_ex = None
    if exclude is not None:
        exclude = [int(e) for e in (exclude.tolist() if hasattr(exclude, "tolist") else exclude)]
        if len(exclude) != len(targets):
            raise ValueError("%s: exclude has %d entries for %d targets" % (who, len(exclude), len(targets)))
        c_ex = (C.c_int * len(exclude))(*exclude)
    return (C.c_float * len(targets))(*targets), c_ex, len(targets), int(radius), int(nearer)


def _warp_out(T: int, V: int, U: int, C_: int, device, hit, depth, src, count, colour, err, rows) -> tuple[Warp, _lib.RslfViewWarpOut]:
    new = lambda shape, dtype, on: torch.empty(shape, dtype=dtype, device=device) if on else None
    out = Warp(new((T, V, U), torch.uint8, hit), new((T, V, U), torch.float32, depth), new((T, V, U), torch.int32, src),
               new((T, V, U), torch.int32, src), new((T, V, U), torch.int32, count), new((T, V, U, C_), torch.float32, colour),
               new((T, V, U), torch.float32, err), new((T, V), torch.float64, rows and err), new((T, V), torch.int32, rows))
    return out, _lib.RslfViewWarpOut(*(None if t is None else t.data_ptr() for t in out))


def view_warp(ctx: Context, depth_s_v_u: torch.Tensor, valid_s_v_u: torch.Tensor | None, slope: float, targets, exclude=None,
              radius: int = 0, nearer: int = 1, volume: "Volume | None" = None, hit: bool = True, depth: bool = True, src: bool = True,
              count: bool = False, colour: bool | None = None, err: bool = False, rows: bool = False) -> Warp:
    """rslf_view_warp (not in the reference): what the view positions `targets` (floats, each finite and within +-65536; they
    need not be integral or inside [0, S - 1]) look like given the disparity planes depth_s_v_u [S, V, U] f32 and
    valid_s_v_u ([S, V, U] u8, or None for every pixel) -- every source pixel is sent to its column in the target, and of the
    pixels that meet in a column the NEAREST wins (nearer=+1: the largest disparity; -1: the smallest), then the nearest
    view, then the smaller view index.  exclude: per target a view that does not take part (-1 / None: nobody); radius > 0:
    only views within it.  colour (default: whenever a volume is given) and err need `volume`; err and rows' row_err also need
    every target to be a view index.  Returns a Warp of new tensors.  Queued on the context's stream, not awaited."""
    c_t, c_ex, T, radius, nearer = _warp_args(targets, exclude, radius, nearer, "view_warp")
    S, V, U = _stack_tensors("view_warp", depth_s_v_u, valid_s_v_u)
    colour = volume is not None if colour is None else bool(colour)
    if (colour or err) and volume is None:
        raise ValueError("view_warp: colour and err read the light field: pass volume")
    out, c_out = _warp_out(T, V, U, volume.C if volume is not None else 0, depth_s_v_u.device, hit, depth, src, count, colour, err, rows)
    ctx.use_current_stream()
    check(_lib.lib().rslf_view_warp(ctx._h, _ptr(depth_s_v_u), _ptr(valid_s_v_u), S, V, U, float(slope),
                                    volume._h if volume is not None else None, c_t, c_ex, T, radius, nearer, C.byref(c_out)), "rslf_view_warp")
    return out


def no_view_warp(who: str, what: str = "get_warped_views") -> None:
    """The forms that have no warp getter say so (every multi-device and sharded form is left out)."""
    raise ValueError("%s: %s is not built here: bring the [S, V, U] planes to one device and call view_warp, "
                     "or use Depth2DComputer / fine_to_coarse_run_host(keep=True)" % (who, what))


def _row_sums(row_err: torch.Tensor, row_count: torch.Tensor, plane: torch.Tensor) -> tuple[np.ndarray, np.ndarray]:
    """Per target, from the row sums [T, V] (waits for the stream) -> (mean_abs_error, coverage of a [T, V, U] plane)."""
    err, count = row_err.cpu().numpy(), row_count.cpu().numpy().astype(np.int64).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mae = np.where(count > 0, err.sum(axis=1) / count, np.nan)
    return mae, count / float(plane.shape[1] * plane.shape[2])


def _view_prediction(w: Warp) -> ViewPrediction:
    return ViewPrediction(w.err, w.hit, *_row_sums(w.row_err, w.row_hits, w.hit), w.row_err, w.row_hits)


class NovelView(NamedTuple):
    """The novel view's planes (include/rslf_hip.h, rslf_novel_view, states the rule), per target k of the T targets of a
    call; None where not asked for.  colour [T, V, U, C] f32: the blend of the views that agree with the pixel's disparity
    (where nobody agreed the first view in field, unverified; 0 at holes); depth f32: the disparity of every target pixel,
    the z-buffer's at hits, a bound's at filled pixels, 0 at holes; fill uint8: 0 hole, 1 hit, 2 filled from the left, 3 from
    the right; n_src int32: the views blended; err f32: the residual against the view that was taken; row_err [T, V] f64 /
    row_cov [T, V] int32: the sum of err over a row's pixels with n_src > 0 and their number."""
    colour: Optional[torch.Tensor]
    depth: Optional[torch.Tensor]
    fill: Optional[torch.Tensor]
    n_src: Optional[torch.Tensor]
    err: Optional[torch.Tensor]
    row_err: Optional[torch.Tensor]
    row_cov: Optional[torch.Tensor]


class NovelViewPrediction(NamedTuple):
    """The leave-one-out yardstick of the novel view: err / fill / n_src [T, V, U] on the device, and per target, as numpy
    float64 [T], mean_abs_error = row_err.sum() / row_cov.sum() (NaN where nobody was blended) and coverage = the pixels with
    n_src > 0 over V * U."""
    err: torch.Tensor
    fill: torch.Tensor
    n_src: torch.Tensor
    mean_abs_error: np.ndarray
    coverage: np.ndarray
    row_err: torch.Tensor
    row_cov: torch.Tensor


def _novel_args(targets, exclude, radius, nearer, max_gap, sources, tol, who: str):
    """-> (c_float array, c_int array or None, T, RslfNovelViewParams); the refusals the library would make, by name first."""
    c_t, c_ex, T, radius, nearer = _warp_args(targets, exclude, radius, nearer, who)
    if int(sources) < 1:
        raise ValueError("%s: sources %r: at least one view to blend" % (who, sources))
    tol = float(tol)
    if not tol >= 0.0:   # (a NaN compares false; +inf accepts every ok pixel)
        raise ValueError("%s: tol %r is not a tolerance >= 0" % (who, tol))
    return c_t, c_ex, T, _lib.RslfNovelViewParams(radius, nearer, int(max_gap), int(sources), tol)


def _novel_out(T: int, V: int, U: int, C_: int, device, colour, depth, fill, n_src, err, rows) -> tuple[NovelView, _lib.RslfNovelViewOut]:
    new = lambda shape, dtype, on: torch.empty(shape, dtype=dtype, device=device) if on else None
    out = NovelView(new((T, V, U, C_), torch.float32, colour), new((T, V, U), torch.float32, depth), new((T, V, U), torch.uint8, fill),
                    new((T, V, U), torch.int32, n_src), new((T, V, U), torch.float32, err), new((T, V), torch.float64, rows and err),
                    new((T, V), torch.int32, rows))
    return out, _lib.RslfNovelViewOut(*(None if t is None else t.data_ptr() for t in out))


def novel_view(ctx: Context, depth_s_v_u: torch.Tensor, valid_s_v_u: torch.Tensor | None, volume: "Volume | None", slope: float, targets,
               exclude=None, radius: int = 0, nearer: int = 1, max_gap: int = 0, sources: int = 4, tol: float = float("inf"),
               colour: bool | None = None, depth: bool = True, fill: bool = True, n_src: bool = True, err: bool = False,
               rows: bool = False) -> NovelView:
    """rslf_novel_view (not in the reference): the view positions `targets` as finished images.  view_warp's z-buffer gives
    every target column a hit or nothing; runs without a hit are filled with the disparity of their FARTHER bound (max_gap > 0:
    only runs of at most that many columns), and every pixel that has a disparity gathers its colour backwards along it from
    the views that agree with it within `tol` (the default, +inf, accepts every ok pixel), nearest views first, at most
    `sources` of them, lerped at sub-pixel columns and blended with weights 1 / (1 + distance).  colour (default: whenever a
    volume is given) and err need `volume`; err and rows' row_err also need every target to be a view index.  Returns a
    NovelView of new tensors.  Queued on the context's stream, not awaited."""
    c_t, c_ex, T, params = _novel_args(targets, exclude, radius, nearer, max_gap, sources, tol, "novel_view")
    S, V, U = _stack_tensors("novel_view", depth_s_v_u, valid_s_v_u)
    colour = volume is not None if colour is None else bool(colour)
    if (colour or err) and volume is None:
        raise ValueError("novel_view: colour and err read the light field: pass volume")
    out, c_out = _novel_out(T, V, U, volume.C if volume is not None else 0, depth_s_v_u.device, colour, depth, fill, n_src, err, rows)
    ctx.use_current_stream()
    check(_lib.lib().rslf_novel_view(ctx._h, _ptr(depth_s_v_u), _ptr(valid_s_v_u), S, V, U, float(slope),
                                     volume._h if volume is not None else None, c_t, c_ex, T, C.byref(params), C.byref(c_out)),
          "rslf_novel_view")
    return out


def no_novel_view(who: str, what: str = "get_novel_views") -> None:
    """The forms that have no novel-view getter say so (every multi-device and sharded form is left out)."""
    raise ValueError("%s: %s is not built here: bring the [S, V, U] planes to one device and call novel_view, "
                     "or use Depth2DComputer / fine_to_coarse_run_host(keep=True)" % (who, what))


def _novel_view_prediction(w: NovelView) -> NovelViewPrediction:
    return NovelViewPrediction(w.err, w.fill, w.n_src, *_row_sums(w.row_err, w.row_cov, w.fill), w.row_err, w.row_cov)


def grid_step(dmin: float, dmax: float, dim_d: int, who: str) -> float:
    """One step of the hypothesis grid, (dmax - dmin) / (dim_d - 1): the default tolerance of the consistency getters."""
    if int(dim_d) < 2:
        raise ValueError("%s: dim_d=%d has no grid step: pass tol" % (who, dim_d))
    return (float(dmax) - float(dmin)) / (int(dim_d) - 1)


class Depth2DComputer:
    """rslf::Depth2DComputer<T> (dc.hpp:166-225, :651-805): disparities for every view of the light field,
    visiting the views from the centre outwards and propagating along EPI lines."""

    def __init__(self, epis, dmin: float, dmax: float, dim_d: int, epi_scale_factor: float = -1.0,
                 parameters: Depth1DParameters | None = None, verbose: bool = False, ctx: Context | None = None,
                 subgrid: bool = False, peaks: bool = False, propagation_ratio: float | None = None,
                 u_dilation: int = 1, dilation_kind=DILATE_CUBIC):
        self.m_parameters = parameters or Depth1DParameters.get_default()
        # not in the reference: the EPIs are dilated along u on the device (Volume.dilated_u) and the object behaves bit for
        # bit as if built from the dilated EPIs with par_slope_factor * u_dilation -- sweep, propagation, consistency, warp,
        # novel view and the renderers all answer in the dilated frame, U' wide; undilated() brings a plane back
        self.m_u_dilation, self.m_dilation_kind = _u_dilation(u_dilation, dilation_kind, "Depth2DComputer")
        require_no_line_confidence_dilated(self.m_parameters, self.m_u_dilation, "Depth2DComputer")
        # not in the reference: ambiguous pixels are withheld from propagation (rslf_sweep_propagation_ratio;
        # get_withheld_sources); reads the peak planes
        self.m_propagation_ratio = _propagation_ratio(propagation_ratio, "Depth2DComputer")
        if self.m_propagation_ratio and not peaks:
            raise ValueError("Depth2DComputer: propagation_ratio reads the peak planes: pass peaks=True")
        self.m_withheld: int | None = None
        # not in the reference: run() also fills the winner and the runner-up peak of every scanned or painted pixel
        # (rslf_sweep_peaks; get_peaks_s_v_u)
        self.m_peaks = bool(peaks)
        self.m_peaks_s_v_u: Peaks | None = None
        # not in the reference: every visit's disparities are moved off the hypothesis grid before the median and the
        # propagation (rslf_sweep_subgrid); every getter then shows refined planes
        self.m_subgrid = bool(subgrid)
        if isinstance(epis, Volume):
            self.m_epis = epis
        elif isinstance(epis, (list, tuple)):
            self.m_epis = Volume.from_epis(epis, epi_scale_factor, ctx)
        elif isinstance(epis, np.ndarray):
            a = epis[..., 0] if (epis.ndim == 4 and epis.shape[3] == 1) else epis
            self.m_epis = Volume.from_epis(list(a), epi_scale_factor, ctx)
        else:
            self.m_epis = Volume.from_dense(epis, epi_scale_factor if epi_scale_factor > 0 else 1.0, ctx)
        if self.m_u_dilation != 1:
            self.m_epis = self.m_epis.dilated_u(self.m_u_dilation, self.m_dilation_kind)
            self.m_parameters = _dilated_parameters(self.m_parameters, self.m_u_dilation)
        vol = self.m_epis
        self.m_dim_d, self.m_dmin, self.m_dmax = int(dim_d), float(dmin), float(dmax)
        self.m_accept_all = False
        dev = vol.ctx.device
        S, V, U, C_ = vol.S, vol.V, vol.U, vol.C
        self.m_edge_confidence_s_v_u = torch.empty((S, V, U), dtype=torch.float32, device=dev)
        self.m_edge_confidence_mask_s_v_u = torch.empty((S, V, U), dtype=torch.uint8, device=dev)
        self.m_disp_confidence_s_v_u = torch.empty((S, V, U), dtype=torch.float32, device=dev)
        self.m_best_depth_s_v_u = torch.empty((S, V, U), dtype=torch.float32, device=dev)
        self.m_rbar_s_v_u = torch.empty((S, V, U, C_), dtype=torch.float32, device=dev)
        self.m_scan_mask_s_v_u = torch.empty((S, V, U), dtype=torch.uint8, device=dev)
        # dc.hpp:721-738: allocated in the _USE_LINE_CONFIDENCE_SCORE build only
        self.m_line_confidence_s_v_u = (torch.empty((S, V, U), dtype=torch.float32, device=dev)
                                        if self._line_mode() != LINE_CONF_OFF else None)
        self.stats: RslfStats | None = None

    def _line_mode(self) -> int:
        mode = int(self.m_parameters.par_line_confidence_mode)
        if mode not in (LINE_CONF_OFF, LINE_CONF_AS_BUILT, LINE_CONF_GATE):
            raise ValueError("par_line_confidence_mode=%d: 0 (off), 1 (as built) or 2 (gate)" % mode)
        require_no_line_confidence_dilated(self.m_parameters, self.m_u_dilation, "Depth2DComputer")   # (set after the constructor ran)
        return mode

    def undilated(self, name: str) -> torch.Tensor:
        """A result plane on the source grid, [S, V, U] (rbar [S, V, U, C]): its columns u * u_dilation.  Names: depth,
        valid (get_valid_depths_mask_s_v_u), edge_mask, edge_confidence, disp_confidence, rbar, scan_mask.  With
        u_dilation = 1 the plane itself."""
        planes = dict(depth=self.m_best_depth_s_v_u, edge_mask=self.m_edge_confidence_mask_s_v_u,
                      edge_confidence=self.m_edge_confidence_s_v_u, disp_confidence=self.m_disp_confidence_s_v_u,
                      rbar=self.m_rbar_s_v_u, scan_mask=self.m_scan_mask_s_v_u, valid=None)
        if name == "valid":
            planes["valid"] = self.get_valid_depths_mask_s_v_u()
        return _undilated("Depth2DComputer", planes, name, self.m_epis, ("rbar",))

    def run(self, want_stats: bool = True) -> None:
        """dc.hpp:748-805."""
        vol = self.m_epis
        p = self.m_parameters.to_c()
        st = RslfStats() if want_stats else None
        vol.ctx.use_current_stream()
        args = (vol.ctx._h, vol._h, self.m_dmin, self.m_dmax, self.m_dim_d, C.byref(p), _ptr(self.m_edge_confidence_s_v_u),
                _ptr(self.m_edge_confidence_mask_s_v_u), _ptr(self.m_disp_confidence_s_v_u), _ptr(self.m_best_depth_s_v_u),
                _ptr(self.m_rbar_s_v_u), _ptr(self.m_scan_mask_s_v_u), C.byref(st) if st is not None else None)
        mode = self._line_mode()
        if mode != LINE_CONF_OFF and self.m_line_confidence_s_v_u is None:   # the mode was set after the constructor ran
            self.m_line_confidence_s_v_u = torch.empty_like(self.m_edge_confidence_s_v_u)
        c_pk, ratio = None, 0.0
        if self.m_peaks:
            shape, dev = tuple(self.m_edge_confidence_s_v_u.shape), vol.ctx.device
            self.m_peaks_s_v_u = Peaks(torch.empty(shape, dtype=torch.int32, device=dev), torch.empty(shape, dtype=torch.float32, device=dev),
                                       None, torch.empty(shape, dtype=torch.int32, device=dev),
                                       torch.empty(shape, dtype=torch.float32, device=dev))
            c_pk, ratio = C.byref(_sweep_peak_planes(self.m_peaks_s_v_u, *shape)), self.m_propagation_ratio
            self.m_withheld = None   # read on demand: the count waits for the stream
        # the family's widest entry: a mode that is off goes in neutral, and the call is the narrower entry's
        check(_lib.lib().rslf_depth2d_run_pr(*args, mode, _ptr(self.m_line_confidence_s_v_u), 1 if self.m_subgrid else 0, c_pk, ratio),
              "rslf_depth2d_run_pr")
        self.stats = st

    def _line_gates(self) -> bool:
        """The #ifdef chain (dc.hpp:838-847, :877-888, :901-907): C_d first, then C_l where the `#elseif` branches are taken."""
        return self._line_mode() == LINE_CONF_GATE and not self.m_parameters.par_use_disp_confidence_score

    def get_depths_s_v_u(self) -> torch.Tensor:
        return self.m_best_depth_s_v_u

    def get_peaks_s_v_u(self) -> Peaks:
        """Not in the reference: after run() with peaks=True, the Peaks of [S,V,U] planes on the device -- idx / score (the
        scan's arg max and its score), runner_idx / runner_score (-1 / 0 without another candidate); disp is None.  A pixel no
        visit scanned or painted holds -1 / 0.  (run() refuses dim_d above 2 ** 24 with the mode on; for fields whose later
        visits still scan a large share of a view, Context.set_debug(peaks_list=0) is the faster form.)"""
        if not self.m_peaks:
            raise ValueError("get_peaks_s_v_u: this object was built without peaks=True")
        if self.m_peaks_s_v_u is None:
            raise ValueError("get_peaks_s_v_u: run() first")
        return self.m_peaks_s_v_u

    def get_propagation_ratio(self) -> float:
        return self.m_propagation_ratio

    def get_withheld_sources(self) -> int:
        """Not in the reference: after run(), the sources the sweep withheld from propagation -- pixels that passed the
        reference's gate and whose peaks were ambiguous at propagation_ratio, summed over the visits; 0 without the ratio.
        Waits for the stream the first time.  Another sweep on the same context in between takes the count's place: ask
        before it."""
        if self.m_peaks and self.m_peaks_s_v_u is None:
            raise ValueError("get_withheld_sources: run() first")
        if not self.m_propagation_ratio:
            return 0
        if self.m_withheld is None:
            self.m_withheld = self.m_epis.ctx.get_withheld_sources()
        return self.m_withheld

    def set_accept_all(self, b: bool) -> None:
        self.m_accept_all = bool(b)

    def _confidence_mask_s_v_u(self) -> torch.Tensor:
        """The mask the two getters paint under: m_edge_confidence_mask_s_v_u in the default build (dc.hpp:840-842,
        :885-887); with par_use_disp_confidence_score, C_d > (float)par_disp_score_threshold (:832-834, :875-878)."""
        if self._line_gates():   # dc.hpp:842, :883: C_l > (float)par_line_score_threshold, one comparison on the device
            return (self.m_line_confidence_s_v_u > float(np.float32(self.m_parameters.par_line_score_threshold))).to(torch.uint8) * 255
        if not self.m_parameters.par_use_disp_confidence_score:
            return self.m_edge_confidence_mask_s_v_u
        return (self.m_disp_confidence_s_v_u > float(np.float32(self.m_parameters.par_disp_score_threshold))).to(torch.uint8) * 255

    def get_coloured_epi(self, a_v=-1, lut_bgr=None) -> torch.Tensor:
        """dc.hpp:808-856: the S x U slice of the disparities at scanline a_v (< 0: floor(V / 2.0)), scaled over its own
        min / max, colour-mapped, black outside the mask; no line drawing -> [S, U, 3] uint8 BGR.  The slice is read in
        place through its row stride.  What a NaN disparity gives is unspecified."""
        vol = self.m_epis
        a_v = int(np.floor(vol.V / 2.0)) if a_v < 0 else int(a_v)
        if a_v >= vol.V:
            raise ValueError("scanline %d of %d" % (a_v, vol.V))
        plane, mask = self.m_best_depth_s_v_u[:, a_v, :], self._confidence_mask_s_v_u()[:, a_v, :]
        lo, hi = render_fit(vol.ctx, plane, None, FIT_MINMAX)
        return render_planes(vol.ctx, plane.unsqueeze(0), lo, hi, RENDER_SHIFT, lut_bgr, mask.unsqueeze(0), MASK_BLACK)[0]

    def get_disparity_map(self, a_s=-1, lut_bgr=None) -> torch.Tensor:
        """dc.hpp:858-891: view a_s (< 0: floor(S / 2.0)) scaled over its min / max (every pixel), colour-mapped, black
        outside the mask -> [V, U, 3] uint8 BGR.  What a NaN disparity gives is unspecified."""
        vol = self.m_epis
        a_s = int(np.floor(vol.S / 2.0)) if a_s < 0 else int(a_s)
        if a_s >= vol.S:
            raise ValueError("view %d of %d" % (a_s, vol.S))
        plane, mask = self.m_best_depth_s_v_u[a_s], self._confidence_mask_s_v_u()[a_s]
        lo, hi = render_fit(vol.ctx, plane, None, FIT_MINMAX)
        return render_planes(vol.ctx, plane.unsqueeze(0), lo, hi, RENDER_SHIFT, lut_bgr, mask.unsqueeze(0), MASK_BLACK)[0]

    def _coloured_stack(self, planes: torch.Tensor, mask: torch.Tensor, lut_bgr) -> torch.Tensor:
        ctx = self.m_epis.ctx
        return render_planes_each(ctx, planes, render_fit_many(ctx, planes, None, FIT_MINMAX), RENDER_SHIFT, lut_bgr, mask, MASK_BLACK)

    def get_disparity_maps(self, lut_bgr=None) -> torch.Tensor:
        """get_disparity_map(a_s) for every view a_s (the loop of the reference's demo, tests/test_depth_computation_2d.cpp:77)
        -> [S, V, U, 3] uint8 BGR: one batch of fits and one render launch, each view over its own min / max."""
        return self._coloured_stack(self.m_best_depth_s_v_u, self._confidence_mask_s_v_u(), lut_bgr)

    def get_coloured_epis(self, lut_bgr=None) -> torch.Tensor:
        """get_coloured_epi(a_v) for every scanline a_v -> [V, S, U, 3] uint8 BGR: one batch of fits and one render launch.
        The S x U slices are read in place through their strides; the volume is not copied."""
        return self._coloured_stack(self.m_best_depth_s_v_u.permute(1, 0, 2), self._confidence_mask_s_v_u().permute(1, 0, 2), lut_bgr)

    def get_valid_depths_mask_s_v_u(self) -> torch.Tensor:
        """dc.hpp:893-915, default build: C_e > edge threshold (or everything > -1 with accept_all)."""
        if self._line_gates() and not self.m_accept_all:   # dc.hpp:904
            return (self.m_line_confidence_s_v_u > float(np.float32(self.m_parameters.par_line_score_threshold))).to(torch.uint8) * 255
        thr = -1.0 if self.m_accept_all else float(np.float32(self.m_parameters.par_edge_score_threshold))
        return (self.m_edge_confidence_s_v_u > thr).to(torch.uint8) * 255

    def get_consistency(self, tol: float | None = None, radius: int = 0, min_agree: int = 0, mask: torch.Tensor | None = None,
                        counts: bool = True, fused: bool = True) -> Consistency:
        """Not in the reference: after run(), view_consistency of the disparity planes with the sweep's own slope factor.
        tol=None: one step of the hypothesis grid, (dmax - dmin) / (dim_d - 1); mask=None: get_valid_depths_mask_s_v_u().
        The sweep's planes are read, never written."""
        tol = grid_step(self.m_dmin, self.m_dmax, self.m_dim_d, "get_consistency") if tol is None else tol
        mask = self.get_valid_depths_mask_s_v_u() if mask is None else mask
        return view_consistency(self.m_epis.ctx, self.m_best_depth_s_v_u, mask, float(np.float32(self.m_parameters.par_slope_factor)),
                                tol, radius, min_agree, counts, fused)

    def get_consistent_depths_mask_s_v_u(self, tol: float | None = None, radius: int = 0, min_agree: int = 1,
                                         mask: torch.Tensor | None = None) -> torch.Tensor:
        """Not in the reference: the `valid` plane of get_consistency alone -- 255 where the pixel is in `mask`, its disparity
        is finite and at least min_agree other views agree with it -- [S, V, U] uint8; no other plane is computed."""
        return self.get_consistency(tol, radius, min_agree, mask, counts=False, fused=False).valid

    def get_warped_views(self, targets, mask: torch.Tensor | None = None, radius: int = 0, nearer: int = 1, exclude=None,
                         colour: bool = True, count: bool = False) -> Warp:
        """Not in the reference: after run(), view_warp of the disparity planes with the sweep's own slope factor -- the views
        at the positions `targets` as the other views predict them: hit, depth, src_view, src_col and (colour=True) the
        light field's radiance at the winner.  mask=None: get_valid_depths_mask_s_v_u().  A z-buffer keeps the LARGEST
        disparity that arrives (nearer=1), so one wrong large value wins its pixel: get_consistent_depths_mask_s_v_u() is the
        mask to pass when that matters.  The sweep's planes are read, never written."""
        mask = self.get_valid_depths_mask_s_v_u() if mask is None else mask
        return view_warp(self.m_epis.ctx, self.m_best_depth_s_v_u, mask, float(np.float32(self.m_parameters.par_slope_factor)), targets,
                         exclude, radius, nearer, self.m_epis, count=count, colour=colour)

    def get_view_prediction(self, targets=None, mask: torch.Tensor | None = None, radius: int = 0, nearer: int = 1) -> ViewPrediction:
        """Not in the reference: the leave-one-out yardstick -- every view of `targets` (default: all of them) predicted from
        the disparities and radiances of the OTHER views and compared with the view that was taken: the err and hit planes,
        and per target mean_abs_error (row_err.sum() / row_hits.sum(), NaN where nothing arrived) and coverage (hits over
        V * U).  It judges a mask or a parameter choice without ground-truth depth.  Waits for the stream."""
        targets = list(range(self.m_epis.S)) if targets is None else [int(t) for t in targets]
        mask = self.get_valid_depths_mask_s_v_u() if mask is None else mask
        w = view_warp(self.m_epis.ctx, self.m_best_depth_s_v_u, mask, float(np.float32(self.m_parameters.par_slope_factor)), targets,
                      targets, radius, nearer, self.m_epis, depth=False, src=False, colour=False, err=True, rows=True)
        return _view_prediction(w)

    def get_novel_views(self, targets, mask: torch.Tensor | None = None, radius: int = 0, nearer: int = 1, exclude=None, max_gap: int = 0,
                        sources: int = 4, tol: float | None = None, colour: bool = True) -> NovelView:
        """Not in the reference: after run(), novel_view of the disparity planes with the sweep's own slope factor and the
        light field itself -- the views at the positions `targets` as finished images: colour, depth, fill and n_src.
        mask=None: get_valid_depths_mask_s_v_u(), as get_warped_views; tol=None: one step of the hypothesis grid.  The sweep's
        planes are read, never written."""
        tol = grid_step(self.m_dmin, self.m_dmax, self.m_dim_d, "get_novel_views") if tol is None else tol
        mask = self.get_valid_depths_mask_s_v_u() if mask is None else mask
        return novel_view(self.m_epis.ctx, self.m_best_depth_s_v_u, mask, self.m_epis, float(np.float32(self.m_parameters.par_slope_factor)),
                          targets, exclude, radius, nearer, max_gap, sources, tol, colour=colour)

    def get_novel_view_prediction(self, targets=None, mask: torch.Tensor | None = None, radius: int = 0, nearer: int = 1, max_gap: int = 0,
                                  sources: int = 4, tol: float | None = None) -> NovelViewPrediction:
        """Not in the reference: get_view_prediction with the novel view in the warp's place -- every view of `targets`
        (default: all of them) rendered from the OTHER views and compared with the view that was taken: err, fill and n_src,
        and per target mean_abs_error and coverage over the pixels somebody was blended into.  Waits for the stream."""
        targets = list(range(self.m_epis.S)) if targets is None else [int(t) for t in targets]
        tol = grid_step(self.m_dmin, self.m_dmax, self.m_dim_d, "get_novel_view_prediction") if tol is None else tol
        mask = self.get_valid_depths_mask_s_v_u() if mask is None else mask
        w = novel_view(self.m_epis.ctx, self.m_best_depth_s_v_u, mask, self.m_epis, float(np.float32(self.m_parameters.par_slope_factor)),
                       targets, targets, radius, nearer, max_gap, sources, tol, colour=False, depth=False, err=True, rows=True)
        return _novel_view_prediction(w)

    def results(self) -> dict:
        torch.cuda.synchronize(self.m_epis.ctx.device)
        out = dict(edge_confidence=self.m_edge_confidence_s_v_u.cpu().numpy(),
                   edge_mask=self.m_edge_confidence_mask_s_v_u.cpu().numpy(),
                   disp_confidence=self.m_disp_confidence_s_v_u.cpu().numpy(),
                   depth=self.m_best_depth_s_v_u.cpu().numpy(), rbar=self.m_rbar_s_v_u.cpu().numpy(),
                   scan_mask=self.m_scan_mask_s_v_u.cpu().numpy())
        if self.m_line_confidence_s_v_u is not None:
            out["line_confidence"] = self.m_line_confidence_s_v_u.cpu().numpy()
        if self.m_peaks and self.m_peaks_s_v_u is not None:
            pk = self.m_peaks_s_v_u
            out.update(peak_idx=pk.idx.cpu().numpy(), peak_score=pk.score.cpu().numpy(),
                       peak_runner_idx=pk.runner_idx.cpu().numpy(), peak_runner_score=pk.runner_score.cpu().numpy())
        return out


# ---- "next" row: the single-EPI class -------------------

def compute_1D_depth_epi(vol: Volume, a_dmin_v_u, a_dmax_v_u, a_dim_d: int, a_s_hat: int,
                         a_edge_confidence_v_u: torch.Tensor, a_edge_confidence_mask_v_u: torch.Tensor,
                         a_disp_confidence_v_u: torch.Tensor, a_best_depth_v_u: torch.Tensor, a_rbar_v_u: torch.Tensor,
                         a_parameters: Depth1DParameters | None = None, a_mask_v_u: torch.Tensor | None = None, *,
                         idx_v_u: torch.Tensor | None = None, score_v_u: torch.Tensor | None = None,
                         want_stats: bool = False, subgrid: bool = False) -> RslfStats | None:
    """core.hpp:251-267 for every EPI of the volume: the scan alone, no selective median.  subgrid (not in the reference):
    every disparity the scan writes is moved off the hypothesis grid (subgrid_refine)."""
    p = (a_parameters or Depth1DParameters()).to_c()
    planes = isinstance(a_dmin_v_u, torch.Tensor)
    st = RslfStats() if want_stats else None
    vol.ctx.use_current_stream()
    args = (vol.ctx._h, vol._h, _ptr(a_dmin_v_u if planes else None), _ptr(a_dmax_v_u if planes else None),
            0.0 if planes else float(a_dmin_v_u), 0.0 if planes else float(a_dmax_v_u), a_dim_d, a_s_hat,
            _ptr(a_edge_confidence_v_u), _ptr(a_edge_confidence_mask_v_u), _ptr(a_disp_confidence_v_u),
            _ptr(a_best_depth_v_u), _ptr(a_rbar_v_u), C.byref(p), _ptr(a_mask_v_u), _ptr(idx_v_u), _ptr(score_v_u),
            C.byref(st) if st is not None else None)
    if subgrid:
        check(_lib.lib().rslf_depth_epi_scan_sub(*args, 1), "rslf_depth_epi_scan_sub")
    else:
        check(_lib.lib().rslf_depth_epi_scan(*args), "rslf_depth_epi_scan")
    return st


class Depth1DComputer:
    """rslf::Depth1DComputer<T> (dc.hpp:26-70, :256-371): ONE EPI ([S,U] or [S,U,3], uint8 or float32), edge
    confidence + scan, no median.  Results are [U] CUDA tensors."""

    def __init__(self, epi, dmin: float, dmax: float, dim_d: int, s_hat: int = -1, epi_scale_factor: float = -1.0,
                 parameters: Depth1DParameters | None = None, ctx: Context | None = None, subgrid: bool = False,
                 u_dilation: int = 1, dilation_kind=DILATE_CUBIC):
        self.m_parameters = parameters or Depth1DParameters.get_default()
        self.m_subgrid = bool(subgrid)   # not in the reference: disparities moved off the hypothesis grid (subgrid_refine)
        # not in the reference: the EPI dilated along u on the device, as Depth1DComputer_pile does
        self.m_u_dilation, self.m_dilation_kind = _u_dilation(u_dilation, dilation_kind, "Depth1DComputer")
        self.m_epi = Volume.from_epis([np.asarray(epi)], epi_scale_factor, ctx)
        if self.m_u_dilation != 1:
            self.m_epi = self.m_epi.dilated_u(self.m_u_dilation, self.m_dilation_kind)
            self.m_parameters = _dilated_parameters(self.m_parameters, self.m_u_dilation)
        vol = self.m_epi
        self.m_dim_d, self.m_dmin, self.m_dmax = int(dim_d), float(dmin), float(dmax)
        self.m_s_hat = int(np.floor((0.0 + vol.S) / 2)) if (s_hat < 0 or s_hat > vol.S - 1) else int(s_hat)   # dc.hpp:303-311
        dev = vol.ctx.device
        U, C_ = vol.U, vol.C
        self.m_edge_confidence_u = torch.empty((1, U), dtype=torch.float32, device=dev)
        self.m_edge_confidence_mask_u = torch.empty((1, U), dtype=torch.uint8, device=dev)
        self.m_disp_confidence_u = torch.empty((1, U), dtype=torch.float32, device=dev)
        self.m_best_depth_u = torch.empty((1, U), dtype=torch.float32, device=dev)
        self.m_rbar_u = torch.empty((1, U, C_), dtype=torch.float32, device=dev)
        self.m_depth_idx_u = torch.empty((1, U), dtype=torch.int32, device=dev)
        self.m_score_u = torch.empty((1, U), dtype=torch.float32, device=dev)
        self.stats: RslfStats | None = None

    def run(self) -> None:
        """dc.hpp:325-371."""
        vol = self.m_epi
        p = self.m_parameters.to_c()
        st = RslfStats()
        vol.ctx.use_current_stream()
        args = (vol.ctx._h, vol._h, self.m_dmin, self.m_dmax, self.m_dim_d, self.m_s_hat, C.byref(p),
                _ptr(self.m_edge_confidence_u), _ptr(self.m_edge_confidence_mask_u), _ptr(self.m_disp_confidence_u),
                _ptr(self.m_best_depth_u), _ptr(self.m_rbar_u), _ptr(self.m_depth_idx_u), _ptr(self.m_score_u), C.byref(st))
        if self.m_subgrid:
            check(_lib.lib().rslf_depth1d_run_sub(*args, 1), "rslf_depth1d_run_sub")
        else:
            check(_lib.lib().rslf_depth1d_run(*args), "rslf_depth1d_run")
        self.stats = st
        self._ran = True

    def get_coloured_epi(self, lut_bgr=None) -> torch.Tensor:
        """dc.hpp:374-416: as Depth1DComputer_pile.get_coloured_epi for the one EPI -> [S, U, 3] uint8 BGR.  This class
        tests `requested_index > 0` where the pile tests `> -1` (:401 against :601): column 0 is never painted, and no
        other column depends on it, so it is the pile's picture with column 0 black."""
        vol = self.m_epi
        out = _coloured_epi_rows(vol.ctx, self.m_best_depth_u, self.m_edge_confidence_mask_u, vol.S, self.m_s_hat, 0, lut_bgr)
        out[:, 0, :] = 0
        return out

    def undilated(self, name: str) -> torch.Tensor:
        """A result plane on the source grid, [U] (rbar [U, C]).  Names: depth, valid (the edge mask), edge_confidence,
        disp_confidence, rbar, depth_idx, score."""
        planes = dict(depth=self.m_best_depth_u, valid=self.m_edge_confidence_mask_u, edge_confidence=self.m_edge_confidence_u,
                      disp_confidence=self.m_disp_confidence_u, rbar=self.m_rbar_u, depth_idx=self.m_depth_idx_u, score=self.m_score_u)
        return _undilated("Depth1DComputer", planes, name, self.m_epi, ("rbar",))[0]

    def get_scores_u_d(self) -> torch.Tensor:
        """After run(): the EPI's [U, D] score matrix, the reference's buf_scores_u_d (core.hpp:616-625), over the pixels
        that received a disparity (the final edge-confidence mask); other rows are 0."""
        if not getattr(self, "_ran", False):
            raise RuntimeError("get_scores_u_d shows the pixels run() gave a disparity: call run() first")
        return compute_1D_depth_scores(self.m_epi, self.m_dmin, self.m_dmax, self.m_dim_d, self.m_s_hat, self.m_parameters,
                                       self.m_edge_confidence_mask_u)[0]

    def get_peaks_u(self) -> Peaks:
        """After run(): the EPI's peaks (Depth1DComputer_pile.get_peaks), [U] each."""
        if not getattr(self, "_ran", False):
            raise RuntimeError("get_peaks_u shows the pixels run() gave a disparity: call run() first")
        return Peaks(*(t[0] for t in compute_1D_depth_peaks(self.m_epi, self.m_dmin, self.m_dmax, self.m_dim_d, self.m_s_hat,
                                                            self.m_parameters, self.m_edge_confidence_mask_u)))

    def results(self) -> dict:
        torch.cuda.synchronize(self.m_epi.ctx.device)
        return dict(edge_confidence=self.m_edge_confidence_u[0].cpu().numpy(), edge_mask=self.m_edge_confidence_mask_u[0].cpu().numpy(),
                    disp_confidence=self.m_disp_confidence_u[0].cpu().numpy(), depth=self.m_best_depth_u[0].cpu().numpy(),
                    rbar=self.m_rbar_u[0].cpu().numpy(), depth_idx=self.m_depth_idx_u[0].cpu().numpy(),
                    score=self.m_score_u[0].cpu().numpy())


# ---- "next" row: fine-to-coarse ---------------------------

_MIN_SPATIAL_DIM = 10   # rslf_fine_to_coarse.hpp:8


def downsample_EPIs(raw_vsuc: torch.Tensor, ctx: Context | None = None, is_u8: bool = False, dtype=None) -> torch.Tensor:
    """rslf::downsample_EPIs (src/rslf_fine_to_coarse_core.cpp:14-60) on a dense RAW float32 CUDA volume
    [V,S,U,C] -> [V2,S,U2,C].  `dtype` is the light field's element type: np.uint8 (or is_u8=True) -- the values are
    uchar levels of a CV_8U field and the blur and the halving run in uchar arithmetic; np.uint16 -- ushort levels of a
    CV_16U field, each blurred level rounded back to ushort before the halving; float32 (the default) -- float arithmetic.
    The reference's Mats keep the input's own type through the pyramid."""
    dt = np.dtype(np.uint8) if (dtype is None and is_u8) else field_dtype(np.float32 if dtype is None else dtype)
    ctx = ctx or default_context(raw_vsuc.device)
    t = raw_vsuc.contiguous()
    V, S, U, C_ = t.shape
    v2, u2 = C.c_int(), C.c_int()
    check(_lib.lib().rslf_f2c_level_dims(V, U, C.byref(v2), C.byref(u2)), "rslf_f2c_level_dims")
    out = torch.empty((v2.value, S, u2.value, C_), dtype=torch.float32, device=t.device)
    ctx.use_current_stream()
    name = "rslf_downsample_epis_" + _SUFFIX[dt]
    check(getattr(_lib.lib(), name)(ctx._h, _ptr(t), V, S, U, C_, _ptr(out)), name)
    return out


def f2c_level(raw_vsuc: torch.Tensor, dtype, epi_scale_factor: float, ctx: Context) -> tuple[float, torch.Tensor]:
    """The per-level rule of FineToCoarse for a light field of element type `dtype` (f2c_pyramid): the level's epi_scale_factor -- Depth2DComputer's constructor normalises ITS input,
    uchar by 1/255, any other depth by the level's own max unless a factor was given (dc.hpp:671-705) -- and the next
    level, downsampled in the field's own arithmetic (f2c.hpp:145-147).  Returns (scale, next raw level)."""
    dt = field_dtype(dtype)
    if dt == np.uint8:
        scale = 255.0
    elif epi_scale_factor < 0:
        mx = C.c_float()
        ctx.use_current_stream()
        check(_lib.lib().rslf_device_max_f32(ctx._h, _ptr(raw_vsuc), raw_vsuc.numel(), C.byref(mx)), "rslf_device_max_f32")
        scale = float(mx.value)
    else:
        scale = float(epi_scale_factor)
    return scale, downsample_EPIs(raw_vsuc, ctx, dtype=dt)


def f2c_input(epis, ctx: Context) -> tuple[torch.Tensor, np.dtype]:
    """FineToCoarse's input -- a list of V arrays [S,U] / [S,U,3] or a dense array [V,S,U(,C)] -- as the raw float32 volume
    [V,S,U,C] on the context's device, and the element type its pyramid keeps (field_dtype)."""
    a = np.stack([np.asarray(e) for e in epis]) if isinstance(epis, (list, tuple)) else np.asarray(epis)
    if a.ndim == 3:
        a = a[..., None]
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(ctx.device), field_dtype(a.dtype)


def derivative_channels(ctx: Context, raw_vsuc: torch.Tensor, weight: float, dtype=np.float32) -> torch.Tensor:
    """A dense RAW one-channel level [V,S,U] / [V,S,U,1] (float32 CUDA; f2c_input's output) as the three-channel level
    [V,S,U,3] of (x, fu, fv) (rslf_derivative_channels_dense).  `dtype` is the light field's element type: float32 -- the
    features are capped at max(the level's maximum, 0); np.uint8 / np.uint16 -- the values are integer levels, the features
    are rounded to integers (ties to even) and capped at 255 / 65535."""
    w = _derivative_weight(weight, "derivative_channels")
    if w == 0.0:
        raise ValueError("derivative_channels: derivative_channels %r is not a finite weight > 0" % (weight,))
    dt = field_dtype(dtype)
    if not raw_vsuc.is_cuda or raw_vsuc.dtype != torch.float32:
        raise ValueError("derivative_channels needs a float32 CUDA tensor")
    if raw_vsuc.dim() == 4 and raw_vsuc.shape[3] == 1:
        raw_vsuc = raw_vsuc[..., 0]
    if raw_vsuc.dim() != 3:
        raise ValueError("derivative_channels: a one-channel level [V,S,U] or [V,S,U,1], not %s" % (tuple(raw_vsuc.shape),))
    t = raw_vsuc.contiguous()
    V, S, U = t.shape
    hi = 0.0
    ctx.use_current_stream()
    if dt == np.float32:
        mx = C.c_float()
        check(_lib.lib().rslf_device_max_f32(ctx._h, _ptr(t), t.numel(), C.byref(mx)), "rslf_device_max_f32")
        hi = max(float(mx.value), 0.0)
    out = torch.empty((V, S, U, 3), dtype=torch.float32, device=t.device)
    check(_lib.lib().rslf_derivative_channels_dense(ctx._h, _ptr(t), _ELEM[np.dtype(dt)], V, S, U, w, hi, _ptr(out)),
          "rslf_derivative_channels_dense")
    return out


_derivative_channels_dense = derivative_channels   # (for the callers whose own argument has the name)


def equalize_views(ctx: Context, raw_vsuc: torch.Tensor, mode: int = EQUALIZE_AFFINE, ref_view=None, joint=None,
                   max_gain: float = 4.0, dtype=np.float32, inplace: bool = False) -> tuple[torch.Tensor, np.ndarray]:
    """A dense RAW level [V,S,U] / [V,S,U,C] (float32 CUDA; f2c_input's output) equalised per view (rslf_equalize_views_dense;
    Volume.equalized_views has the rule).  `dtype` is the light field's element type: float32 -- the cap is the level's
    maximum; np.uint8 / np.uint16 -- the values are integer levels, the result is rounded to integers (ties to even) and
    capped at 255 / 65535.  inplace: the tensor itself is equalised (it must be contiguous) and returned.  Returns
    (the level, view_gains [S, C, 2])."""
    m = _equalize_mode(mode, "equalize_views")
    if m == 0:
        raise ValueError("equalize_views: equalize_views %r is not EQUALIZE_GAIN or EQUALIZE_AFFINE" % (mode,))
    dt = field_dtype(dtype)
    if not raw_vsuc.is_cuda or raw_vsuc.dtype != torch.float32:
        raise ValueError("equalize_views needs a float32 CUDA tensor")
    if raw_vsuc.dim() not in (3, 4) or (raw_vsuc.dim() == 4 and raw_vsuc.shape[3] not in (1, 3)):
        raise ValueError("equalize_views: a level [V,S,U], [V,S,U,1] or [V,S,U,3], not %s" % (tuple(raw_vsuc.shape),))
    V, S, U = raw_vsuc.shape[:3]
    C_ = raw_vsuc.shape[3] if raw_vsuc.dim() == 4 else 1
    ref, j, g = _equalize_args(S, C_, ref_view, joint, max_gain, "equalize_views")
    if inplace:
        if not raw_vsuc.is_contiguous():
            raise ValueError("equalize_views: inplace needs a contiguous tensor")
        t = raw_vsuc
    else:
        t = raw_vsuc.clone(memory_format=torch.contiguous_format)
    hi = 0.0
    ctx.use_current_stream()
    if dt == np.float32:
        mx = C.c_float()
        check(_lib.lib().rslf_device_max_f32(ctx._h, _ptr(t), t.numel(), C.byref(mx)), "rslf_device_max_f32")
        hi = float(mx.value)
    a_b = np.zeros((S, C_, 2), np.float32)
    check(_lib.lib().rslf_equalize_views_dense(ctx._h, _ptr(t), _ELEM[np.dtype(dt)], V, S, U, C_, hi, m, ref, j, g, a_b.ctypes.data),
          "rslf_equalize_views_dense")
    return t, a_b


_equalize_views_dense = equalize_views   # (for the callers whose own argument has the name)


def f2c_line_mode(parameters: Depth1DParameters, line_confidence_mode: int | None, who: str) -> int:
    """The line mode of a pyramid.  None: no line confidence, and parameters that ask for one are refused (the paths that
    do not carry C_l).  0 / 1 / 2: that mode on every level; parameters.par_line_confidence_mode must be 0 or equal to it."""
    if line_confidence_mode is None:
        require_no_line_confidence(parameters, who)
        return LINE_CONF_OFF
    mode = int(line_confidence_mode)
    if mode not in (LINE_CONF_OFF, LINE_CONF_AS_BUILT, LINE_CONF_GATE):
        raise ValueError("%s: line_confidence_mode=%d: 0 (off), 1 (as built) or 2 (gate)" % (who, mode))
    if int(parameters.par_line_confidence_mode) not in (LINE_CONF_OFF, mode):
        raise ValueError("%s: par_line_confidence_mode=%d disagrees with line_confidence_mode=%d"
                         % (who, int(parameters.par_line_confidence_mode), mode))
    return mode


def f2c_pyramid(raw: torch.Tensor, dtype, epi_scale_factor: float, parameters: Depth1DParameters, max_pyr_depth: int, ctx: Context,
                line_confidence_mode: int | None = None):
    """The levels of FineToCoarse's constructor (f2c.hpp:103-159), finest first, each built as it is asked for:
    (V, U, the parameters with the level's slope factor and line mode, the level's scale, its raw volume [V,S,U,C])."""
    mode = f2c_line_mode(parameters, line_confidence_mode, "FineToCoarse")
    start_dim_u = raw.shape[2]
    if max_pyr_depth < 1:
        max_pyr_depth = 1 << 30
    counter = 0
    while raw.shape[0] > _MIN_SPATIAL_DIM and raw.shape[2] > _MIN_SPATIAL_DIM and counter < max_pyr_depth:   # f2c.hpp:130
        counter += 1
        par = copy.copy(parameters)
        par.par_slope_factor = float(np.float32((0.0 + raw.shape[2]) / start_dim_u))                     # f2c.hpp:139
        par.par_line_confidence_mode = mode
        scale, nxt = f2c_level(raw, dtype, epi_scale_factor, ctx)
        yield raw.shape[0], raw.shape[2], par, scale, raw
        raw = nxt                                                                                       # f2c.hpp:145-147
    if counter == 0:
        raise ValueError("light field smaller than _MIN_SPATIAL_DIM: no pyramid level")


def f2c_ranges(ctx: Context, depth_up: torch.Tensor, valid_up: torch.Tensor, V: int, U: int, d_min: float,
               d_max: float) -> tuple[torch.Tensor, torch.Tensor]:
    """The per-pixel hypothesis ranges [S,V,U] of a level below the finest: [d_min, d_max] tightened around the valid
    disparities of the level above, depth_up / valid_up [S,V_up,U_up] (f2c.hpp:202-294)."""
    S, V_up, U_up = depth_up.shape
    lo = torch.full((S, V, U), d_min, dtype=torch.float32, device=ctx.device)
    hi = torch.full((S, V, U), d_max, dtype=torch.float32, device=ctx.device)
    ctx.use_current_stream()
    check(_lib.lib().rslf_f2c_tighten_bounds(ctx._h, _ptr(depth_up), _ptr(valid_up), S, V_up, U_up, _ptr(lo), _ptr(hi), V, U),
          "rslf_f2c_tighten_bounds")
    return lo, hi


def f2c_fuse(ctx: Context, depths: Sequence[torch.Tensor], valids: Sequence[torch.Tensor]) -> tuple[torch.Tensor, torch.Tensor]:
    """get_results() (f2c.hpp:302-324): the levels' disparities and validity masks [S,V_p,U_p], finest first, fused from
    coarse to fine -> (out_map_s_v_u [S,V,U] f32, out_validity_s_v_u [S,V,U] u8) at the finest scale."""
    P = len(depths)
    S, V, U = depths[0].shape
    dp = (C.c_void_p * P)(*[t.data_ptr() for t in depths])
    vp = (C.c_void_p * P)(*[t.data_ptr() for t in valids])
    Vp = (C.c_int * P)(*[t.shape[1] for t in depths])
    Up = (C.c_int * P)(*[t.shape[2] for t in depths])
    out_map = torch.empty((S, V, U), dtype=torch.float32, device=ctx.device)
    out_valid = torch.empty((S, V, U), dtype=torch.uint8, device=ctx.device)
    ctx.use_current_stream()
    check(_lib.lib().rslf_f2c_fuse(ctx._h, dp, vp, Vp, Up, P, S, _ptr(out_map), _ptr(out_valid)), "rslf_f2c_fuse")
    return out_map, out_valid


F2C_VALID_COMPAT, F2C_VALID_REFERENCE = 0, 1   # RSLF_F2C_VALID_*
_ELEM = {np.dtype(np.float32): 0, np.dtype(np.uint8): 1, np.dtype(np.uint16): 2}   # RSLF_ELEM_*
_F2C_PLANES = dict(depth=(0, torch.float32), valid=(1, torch.uint8), Ce=(2, torch.float32), Cd=(3, torch.float32),
                   Cl=(4, torch.float32), fused_map=(5, torch.float32), fused_valid=(6, torch.uint8),
                   pk_idx=(7, torch.int32), pk_score=(8, torch.float32), pk_runner_idx=(9, torch.int32),
                   pk_runner_score=(10, torch.float32), fused_pk_idx=(11, torch.int32), fused_pk_score=(12, torch.float32),
                   fused_pk_runner_idx=(13, torch.int32), fused_pk_runner_score=(14, torch.float32),
                   fused_level=(15, torch.uint8))   # RSLF_F2C_PLANE_*
_F2C_GATE_PLANES = dict(cs_agree=(16, torch.int32), cs_seen=(17, torch.int32))   # RSLF_F2C_PLANE_CS_*: the consistency gate's counts


def f2c_consistency_mask(ctx: Context, depth_s_v_u: torch.Tensor, valid_s_v_u: torch.Tensor, slope: float, tol: float, radius: int = 0,
                         min_agree: int = 1, counts: bool = True, dropped: torch.Tensor | None = None):
    """rslf_f2c_consistency_mask (not in the reference): the gate a kept fine-to-coarse run puts on a level's validity.
    depth_s_v_u [S, V, U] f32 and valid_s_v_u [S, V, U] u8 on the context's device; a pixel that is valid with a finite
    disparity becomes 0 in the returned plane unless agree >= min(seen, min_agree), counted as view_consistency counts them;
    every other byte is copied.  Returns (valid_out, agree, seen) as new tensors (agree / seen None with counts=False).
    dropped: a one-element int64 CUDA tensor the launch adds the number of pixels it made invalid to.  Queued, not awaited."""
    tol, radius, min_agree = _consistency_args(tol, radius, min_agree, "f2c_consistency_mask")
    if depth_s_v_u.dim() != 3 or depth_s_v_u.dtype != torch.float32 or not depth_s_v_u.is_cuda or not depth_s_v_u.is_contiguous():
        raise ValueError("f2c_consistency_mask: depth_s_v_u must be a contiguous float32 CUDA tensor [S, V, U]")
    if (valid_s_v_u is None or valid_s_v_u.shape != depth_s_v_u.shape or valid_s_v_u.dtype != torch.uint8 or not valid_s_v_u.is_cuda
            or not valid_s_v_u.is_contiguous()):
        raise ValueError("f2c_consistency_mask: valid_s_v_u must be a contiguous uint8 CUDA tensor of depth_s_v_u's shape")
    if dropped is not None and (dropped.numel() != 1 or dropped.dtype != torch.int64 or not dropped.is_cuda):
        raise ValueError("f2c_consistency_mask: dropped must be a one-element int64 CUDA tensor")
    S, V, U = (int(x) for x in depth_s_v_u.shape)
    out = torch.empty((S, V, U), dtype=torch.uint8, device=depth_s_v_u.device)
    agree = torch.empty((S, V, U), dtype=torch.int32, device=depth_s_v_u.device) if counts else None
    seen = torch.empty((S, V, U), dtype=torch.int32, device=depth_s_v_u.device) if counts else None
    ctx.use_current_stream()
    check(_lib.lib().rslf_f2c_consistency_mask(ctx._h, _ptr(depth_s_v_u), _ptr(valid_s_v_u), S, V, U, float(slope), tol, radius, min_agree,
                                               _ptr(out), _ptr(agree), _ptr(seen), _ptr(dropped)), "rslf_f2c_consistency_mask")
    return out, agree, seen


def _f2c_peak_struct(pk: "Peaks", shape: tuple, who: str) -> _lib.RslfPeaks:
    """The C struct of four peak planes of `shape` (idx / runner_idx int32, score / runner_score f32, all given; disp None)."""
    pk = Peaks(*pk)
    for name, t in zip(Peaks._fields, pk):
        if name == "disp":
            continue
        want = torch.int32 if name.endswith("idx") else torch.float32
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != want or not t.is_cuda or not t.is_contiguous():
            raise ValueError("%s: peaks.%s must be a contiguous %s CUDA tensor of shape %s" % (who, name, want, tuple(shape)))
    return _lib.RslfPeaks(pk.idx.data_ptr(), pk.score.data_ptr(), None, pk.runner_idx.data_ptr(), pk.runner_score.data_ptr())


def f2c_unique_mask(ctx: Context, valid: torch.Tensor, peaks: "Peaks", ratio: float) -> torch.Tensor:
    """rslf_f2c_unique_mask, in place on `valid` (uint8, any shape): a non-zero byte whose pixel has a winner and a runner-up
    with runner_score > ratio * score (one float32 multiply) becomes 0; ratio in (0, 1].  peaks: a Peaks of valid's shape
    (disp None).  Returns valid.  Queued, not awaited."""
    if valid.dtype != torch.uint8 or not valid.is_cuda or not valid.is_contiguous():
        raise ValueError("f2c_unique_mask: valid must be a contiguous uint8 CUDA tensor")
    c_pk = _f2c_peak_struct(peaks, valid.shape, "f2c_unique_mask")
    ctx.use_current_stream()
    check(_lib.lib().rslf_f2c_unique_mask(ctx._h, _ptr(valid), C.byref(c_pk), float(ratio), valid.numel()), "rslf_f2c_unique_mask")
    return valid


def f2c_fuse_peaks(ctx: Context, valids: Sequence[torch.Tensor], peaks: Sequence["Peaks"]) -> tuple["Peaks", torch.Tensor]:
    """rslf_f2c_fuse_peaks: the levels' validity masks and peak planes [S,V_p,U_p], finest first -> (the fused Peaks
    [S,V_0,U_0], fused_level [S,V_0,U_0] uint8): per pixel of the finest plane the first level down the fusion's nearest-pixel
    mask chain whose validity is set, and that pixel's peaks; 255 and -1 / 0 where no level is valid."""
    P = len(valids)
    if P < 1 or len(peaks) != P:
        raise ValueError("f2c_fuse_peaks: one Peaks per level")
    S, V, U = valids[0].shape
    structs = (_lib.RslfPeaks * P)(*[_f2c_peak_struct(pk, v.shape, "f2c_fuse_peaks") for pk, v in zip(peaks, valids)])
    for v in valids:
        if v.dtype != torch.uint8 or not v.is_cuda or not v.is_contiguous() or v.shape[0] != S:
            raise ValueError("f2c_fuse_peaks: every validity plane must be a contiguous uint8 CUDA tensor [S,V_p,U_p]")
    vp = (C.c_void_p * P)(*[t.data_ptr() for t in valids])
    Vp = (C.c_int * P)(*[t.shape[1] for t in valids])
    Up = (C.c_int * P)(*[t.shape[2] for t in valids])
    dev = ctx.device
    out = Peaks(torch.empty((S, V, U), dtype=torch.int32, device=dev), torch.empty((S, V, U), dtype=torch.float32, device=dev), None,
                torch.empty((S, V, U), dtype=torch.int32, device=dev), torch.empty((S, V, U), dtype=torch.float32, device=dev))
    level = torch.empty((S, V, U), dtype=torch.uint8, device=dev)
    c_out = _f2c_peak_struct(out, (S, V, U), "f2c_fuse_peaks")
    ctx.use_current_stream()
    check(_lib.lib().rslf_f2c_fuse_peaks(ctx._h, vp, structs, Vp, Up, P, S, C.byref(c_out), _ptr(level)), "rslf_f2c_fuse_peaks")
    return out, level


class KeptFineToCoarse:
    """rslf_f2c_run: a finished fine-to-coarse run held on the device by the library (fine_to_coarse_run_host(keep=True)).
    Every level's disparities, validity, C_e, C_d (C_l with a line mode) and -- with keep_volumes -- normalised volume, and
    the fused planes, stay where they were computed; planes come out by copy into tensors of the caller's, and the three
    coloured getters of rslf::FineToCoarse are rendered from the kept planes.  `ctx` is the context copies and renders are
    queued on: any context of the run's device."""

    def __init__(self, handle, ctx: Context, stats: RslfStats, grid: tuple | None = None):
        self._h, self.ctx, self.stats = handle, ctx, stats
        self.grid = grid   # (d_min, d_max, dim_d) the run was made with: get_consistency's default tolerance
        d = self.describe()
        self.S, self.C, self.n_levels = d.S, d.C, d.n_levels
        self.dims = [(d.V[l], d.U[l]) for l in range(d.n_levels)]            # (V_p, U_p), finest first
        self.scales = [float(d.epi_scale_factor[l]) for l in range(d.n_levels)]
        self.line_mode, self.validity_rule, self.keep_volumes = d.line_mode, d.validity_rule, bool(d.keep_volumes)
        self.subgrid = bool(_lib.lib().rslf_f2c_run_subgrid(self._h))   # every level was swept in the sub-grid mode
        self.peaks = bool(_lib.lib().rslf_f2c_run_peaks(self._h))       # the run holds peak planes (get_peaks, get_fused_peaks)
        self.uniqueness_ratio = float(_lib.lib().rslf_f2c_run_uniqueness(self._h))   # 0.0: validity by uniqueness was off
        self.propagation_ratio = float(_lib.lib().rslf_f2c_run_propagation_ratio(self._h))   # 0.0: the sweeps were not gated
        tol, radius, min_agree = C.c_float(), C.c_int(), C.c_int()
        check(_lib.lib().rslf_f2c_run_consistency_gate(self._h, C.byref(tol), C.byref(radius), C.byref(min_agree)), "rslf_f2c_run_consistency_gate")
        # (tol, radius, min_agree) of the validity by cross-view consistency, None: the run was made without it
        self.consistency_gate = (float(tol.value), int(radius.value), int(min_agree.value)) if min_agree.value else None
        factor, kind = C.c_int(), C.c_int()
        check(_lib.lib().rslf_f2c_run_level_dilation(self._h, C.byref(factor), C.byref(kind)), "rslf_f2c_run_level_dilation")
        # (factor, kind) of the level dilation the sweeps ran with; (1, DILATE_CUBIC): none.  Every plane is on the level's grid
        self.level_dilation = (int(factor.value), int(kind.value))
        mode, ref = C.c_int(), C.c_int()
        check(_lib.lib().rslf_f2c_run_equalize(self._h, C.byref(mode), C.byref(ref), None), "rslf_f2c_run_equalize")
        # the per-view equalisation the finest level's upload went through: (mode, ref_view), None: the run was made without it
        self.equalize_views = (int(mode.value), int(ref.value)) if mode.value else None
        self._view_gains = None

    @property
    def view_gains(self):
        """The [S, C, 2] float32 (a, b) the run's equalisation applied, C the field's own channel count; None: the run was
        made without it."""
        if self.equalize_views is None:
            return None
        if self._view_gains is None:
            C_ = int(_lib.lib().rslf_f2c_run_view_gains_channels(self._h))   # (the run says how many floats it writes)
            a_b = np.zeros((self.S, C_, 2), np.float32)
            check(_lib.lib().rslf_f2c_run_equalize(self._h, None, None, a_b.ctypes.data), "rslf_f2c_run_equalize")
            self._view_gains = a_b
        return self._view_gains

    def describe(self) -> "_lib.RslfF2cRunDesc":
        d = _lib.RslfF2cRunDesc()
        check(_lib.lib().rslf_f2c_run_describe(self._h, C.byref(d)), "rslf_f2c_run_describe")
        return d

    def plane(self, level: int, name: str) -> torch.Tensor:
        """One kept plane as a new tensor on the device: "depth", "valid", "Ce", "Cd", "Cl" of a level [S,V_p,U_p], or
        "fused_map" / "fused_valid" (level 0); of a run made with peaks=True also "pk_idx", "pk_score", "pk_runner_idx",
        "pk_runner_score" of a level and "fused_pk_*" / "fused_level" (level 0); of a run made with the consistency gate also
        "cs_agree" / "cs_seen" of a gated level."""
        which, dtype = _F2C_GATE_PLANES[name] if name in _F2C_GATE_PLANES else _F2C_PLANES[name]
        if not 0 <= level < self.n_levels:
            raise ValueError("level %d of %d" % (level, self.n_levels))
        out = torch.empty((self.S,) + self.dims[level], dtype=dtype, device=self.ctx.device)
        self.ctx.use_current_stream()
        check(_lib.lib().rslf_f2c_run_copy(self._h, level, which, _ptr(out), 0, self.ctx._h), "rslf_f2c_run_copy")
        return out

    def volume_desc(self, level: int) -> RslfVolumeDesc:
        """rslf_volume_describe of a level's kept volume (the slab stays the run's)."""
        vol, d = C.c_void_p(), RslfVolumeDesc()
        check(_lib.lib().rslf_f2c_run_volume(self._h, level, C.byref(vol)), "rslf_f2c_run_volume")
        check(_lib.lib().rslf_volume_describe(vol, C.byref(d)), "rslf_volume_describe")
        return d

    def get_results(self) -> tuple[torch.Tensor, torch.Tensor]:
        """f2c.hpp:302-324 -> (out_map_s_v_u [S,V,U] f32, out_validity_s_v_u [S,V,U] u8), copies of the kept fused planes."""
        return self.plane(0, "fused_map"), self.plane(0, "fused_valid")

    def get_peaks(self, level: int) -> "Peaks":
        """Not in the reference: a level's four peak planes [S,V_p,U_p] as a Peaks (disp None: the sub-grid value lives in the
        depth plane) -- idx / score the winner, runner_idx / runner_score the runner-up, -1 / 0 where no visit scanned or
        painted the pixel.  Needs a run made with peaks=True."""
        if not self.peaks:
            raise ValueError("get_peaks: this run was made without peaks=True")
        return Peaks(self.plane(level, "pk_idx"), self.plane(level, "pk_score"), None, self.plane(level, "pk_runner_idx"),
                     self.plane(level, "pk_runner_score"))

    def withheld(self, level: int) -> int:
        """Not in the reference: the sources the sweep of `level` withheld from propagation (propagation_ratio); 0 on every
        level of a run made without the ratio."""
        n = C.c_ulonglong()
        check(_lib.lib().rslf_f2c_run_withheld(self._h, int(level), C.byref(n)), "rslf_f2c_run_withheld")
        return int(n.value)

    def inconsistent(self, level: int) -> int:
        """Not in the reference: the pixels the consistency gate made invalid on `level`; 0 on a level accepted whole and on
        every level of a run made without the gate."""
        n = C.c_ulonglong()
        check(_lib.lib().rslf_f2c_run_inconsistent(self._h, int(level), C.byref(n)), "rslf_f2c_run_inconsistent")
        return int(n.value)

    def get_gate_counts(self, level: int) -> tuple[torch.Tensor, torch.Tensor]:
        """Not in the reference: (agree, seen) [S,V_p,U_p] int32, the consistency gate's own counts on `level` at gate time --
        they explain a drop: agree < min(seen, min_agree).  get_consistency afterwards reads the gated validity and counts
        differently.  Needs a run made with the gate, and a level it touched (not the one accepted whole)."""
        if self.consistency_gate is None:
            raise ValueError("get_gate_counts: this run was made without consistency_min_agree")
        return self.plane(level, "cs_agree"), self.plane(level, "cs_seen")

    def get_fused_peaks(self) -> tuple["Peaks", torch.Tensor]:
        """Not in the reference: (Peaks [S,V,U], fused_level [S,V,U] uint8) at the finest size -- for every pixel of the fused
        map the level that decided it (255: none) and the peaks of the pixel of that level it was taken from: the NEAREST
        pixel down the fusion's mask chain, while the fused disparity of a pixel decided by a coarser level is a bilinear
        blend and a 3 x 3 median away from it."""
        if not self.peaks:
            raise ValueError("get_fused_peaks: this run was made without peaks=True")
        return (Peaks(self.plane(0, "fused_pk_idx"), self.plane(0, "fused_pk_score"), None, self.plane(0, "fused_pk_runner_idx"),
                      self.plane(0, "fused_pk_runner_score")), self.plane(0, "fused_level"))

    def get_consistency(self, level: int = 0, fused_result: bool = True, tol: float | None = None, radius: int = 0,
                        min_agree: int = 0, counts: bool = True, fused: bool = True) -> Consistency:
        """Not in the reference: rslf_f2c_run_consistency -- view_consistency of a kept plane pair, read in place: the fused
        map and its validity (fused_result=True, which needs level 0) or a level's depth / valid planes, with the slope
        factor the level's sweep propagated with.  tol=None: one step of the run's hypothesis grid.  Returns a Consistency
        of new [S, V_p, U_p] tensors; the run's planes are not written."""
        self._kept_pair("get_consistency", level, fused_result)
        tol, radius, min_agree = _consistency_args(self._grid_tol("get_consistency", tol), radius, min_agree, "get_consistency")
        out, c_counts = _consistency_out((self.S,) + self.dims[level], self.ctx.device, counts, fused)
        self.ctx.use_current_stream()
        check(_lib.lib().rslf_f2c_run_consistency(self._h, self.ctx._h, int(level), 1 if fused_result else 0, tol, radius, min_agree,
                                                  C.byref(c_counts), _ptr(out.fused), _ptr(out.valid)), "rslf_f2c_run_consistency")
        return out

    def _kept_pair(self, who: str, level: int, fused_result: bool, needs_volume: bool = False) -> None:
        """The refusals every getter of a kept plane pair shares: the level, the fused planes' level, the volume not kept."""
        if not 0 <= level < self.n_levels:
            raise ValueError("level %d of %d" % (level, self.n_levels))
        if fused_result and level != 0:
            raise ValueError("%s: the fused planes are at the finest size: level 0, or fused_result=False" % who)
        if needs_volume and not self.keep_volumes:
            raise ValueError("%s: colour and err read the level's volume: this run was made without keep_volumes" % who)

    def _grid_tol(self, who: str, tol):
        """tol, or for None one step of the run's hypothesis grid."""
        if tol is not None:
            return tol
        if self.grid is None:
            raise ValueError("%s: this object does not know the run's hypothesis grid: pass tol" % who)
        return grid_step(*self.grid, who)

    def _view_warp(self, who: str, targets, exclude, level: int, fused_result: bool, radius: int, nearer: int, **planes) -> Warp:
        self._kept_pair(who, level, fused_result, planes["colour"] or planes["err"])
        c_t, c_ex, T, radius, nearer = _warp_args(targets, exclude, radius, nearer, who)
        out, c_out = _warp_out(T, *self.dims[level], self.C, self.ctx.device, **planes)
        self.ctx.use_current_stream()
        check(_lib.lib().rslf_f2c_run_view_warp(self._h, self.ctx._h, int(level), 1 if fused_result else 0, c_t, c_ex, T, radius, nearer,
                                                C.byref(c_out)), "rslf_f2c_run_view_warp")
        return out

    def get_warped_views(self, targets, level: int = 0, fused_result: bool = True, radius: int = 0, nearer: int = 1, exclude=None,
                         colour: bool | None = None, count: bool = False) -> Warp:
        """Not in the reference: rslf_f2c_run_view_warp -- view_warp of a kept plane pair, read in place: the fused map and its
        validity (fused_result=True, which needs level 0) or a level's depth / valid planes, with the slope factor the level's
        sweep ran with and the level's kept volume.  colour=None: whenever the run keeps its volumes.  A z-buffer keeps the
        largest disparity that arrives (nearer=1), so one wrong large value wins its pixel.  Returns a Warp of new
        [T, V_p, U_p] tensors; the run's planes are not written."""
        colour = self.keep_volumes if colour is None else bool(colour)
        return self._view_warp("get_warped_views", targets, exclude, level, fused_result, radius, nearer, hit=True, depth=True, src=True,
                               count=count, colour=colour, err=False, rows=False)

    def get_view_prediction(self, targets=None, level: int = 0, fused_result: bool = True, radius: int = 0,
                            nearer: int = 1) -> ViewPrediction:
        """Not in the reference: the leave-one-out yardstick of Depth2DComputer.get_view_prediction on a kept plane pair; needs
        a run made with keep_volumes.  Waits for the stream."""
        targets = list(range(self.S)) if targets is None else [int(t) for t in targets]
        return _view_prediction(self._view_warp("get_view_prediction", targets, targets, level, fused_result, radius, nearer, hit=True,
                                                depth=False, src=False, count=False, colour=False, err=True, rows=True))

    def _novel_view(self, who: str, targets, exclude, level: int, fused_result: bool, radius: int, nearer: int, max_gap: int, sources: int,
                    tol, **planes) -> NovelView:
        self._kept_pair(who, level, fused_result, planes["colour"] or planes["err"])
        c_t, c_ex, T, params = _novel_args(targets, exclude, radius, nearer, max_gap, sources, self._grid_tol(who, tol), who)
        out, c_out = _novel_out(T, *self.dims[level], self.C, self.ctx.device, **planes)
        self.ctx.use_current_stream()
        check(_lib.lib().rslf_f2c_run_novel_view(self._h, self.ctx._h, int(level), 1 if fused_result else 0, c_t, c_ex, T, C.byref(params),
                                                 C.byref(c_out)), "rslf_f2c_run_novel_view")
        return out

    def get_novel_views(self, targets, level: int = 0, fused_result: bool = True, radius: int = 0, nearer: int = 1, exclude=None,
                        max_gap: int = 0, sources: int = 4, tol: float | None = None, colour: bool | None = None) -> NovelView:
        """Not in the reference: rslf_f2c_run_novel_view -- novel_view of a kept plane pair, read in place, as get_warped_views
        reads it, with the level's kept volume.  colour=None: whenever the run keeps its volumes; tol=None: one step of the
        run's hypothesis grid.  Returns a NovelView of new [T, V_p, U_p] tensors; the run's planes are not written."""
        colour = self.keep_volumes if colour is None else bool(colour)
        return self._novel_view("get_novel_views", targets, exclude, level, fused_result, radius, nearer, max_gap, sources, tol,
                                colour=colour, depth=True, fill=True, n_src=True, err=False, rows=False)

    def get_novel_view_prediction(self, targets=None, level: int = 0, fused_result: bool = True, radius: int = 0, nearer: int = 1,
                                  max_gap: int = 0, sources: int = 4, tol: float | None = None) -> NovelViewPrediction:
        """Not in the reference: Depth2DComputer.get_novel_view_prediction on a kept plane pair; needs a run made with
        keep_volumes.  Waits for the stream."""
        targets = list(range(self.S)) if targets is None else [int(t) for t in targets]
        return _novel_view_prediction(self._novel_view("get_novel_view_prediction", targets, targets, level, fused_result, radius, nearer,
                                                       max_gap, sources, tol, colour=False, depth=False, fill=True, n_src=True, err=True,
                                                       rows=True))

    def _render(self, name: str, shapes, *args, lut_bgr=None, stacked: bool = False):
        table = _table(lut_bgr)
        outs = [torch.empty(tuple(sh) + (3,), dtype=torch.uint8, device=self.ctx.device) for sh in shapes]
        dst = _ptr(outs[0]) if stacked else (C.c_void_p * len(outs))(*[t.data_ptr() for t in outs])
        self.ctx.use_current_stream()
        st = getattr(_lib.lib(), name)(self._h, self.ctx._h, *args, table.ctypes.data_as(C.c_void_p), dst)
        if st == -1:   # the getters' index rules and the missing volumes
            raise ValueError(_lib.lib().rslf_last_error().decode(errors="replace"))
        check(st, name)
        return outs[0] if stacked else outs

    def get_coloured_depth_maps(self, lut_bgr=None, saturate: bool = True) -> torch.Tensor:
        """f2c.hpp:325-378 as FineToCoarse.get_coloured_depth_maps -> [S, V, U, 3] uint8 BGR."""
        return self._render("rslf_f2c_run_render_depth_maps", [(self.S,) + self.dims[0]], 1 if saturate else 0, lut_bgr=lut_bgr, stacked=True)

    def get_coloured_depth_pyr(self, s: int = -1, lut_bgr=None, saturate: bool = True) -> list:
        """f2c.hpp:491-519 as FineToCoarse.get_coloured_depth_pyr -> a list of [V_p, U_p, 3] uint8 BGR."""
        return self._render("rslf_f2c_run_render_depth_pyr", self.dims, int(s), 1 if saturate else 0, lut_bgr=lut_bgr)

    def get_coloured_epi_pyr(self, v: int = -1, lut_bgr=None, saturate: bool = True) -> list:
        """f2c.hpp:432-488 as FineToCoarse.get_coloured_epi_pyr -> a list of [S, U_p, 3] uint8 BGR."""
        return self._render("rslf_f2c_run_render_epi_pyr", [(self.S, u) for _, u in self.dims], int(v), 1 if saturate else 0, lut_bgr=lut_bgr)

    def close(self) -> None:
        if getattr(self, "_h", None) and not sys.is_finalizing():
            _lib.lib().rslf_f2c_run_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def fine_to_coarse_run_host(epis, d_min: float, d_max: float, dim_d: int, epi_scale_factor: float = -1.0,
                            parameters: Depth1DParameters | None = None, max_pyr_depth: int = -1, accept_all_last_scale: bool = True,
                            ctx: Context | None = None, line_mode: int = LINE_CONF_OFF, want_levels: bool = False, keep: bool = False,
                            validity_rule: int = F2C_VALID_COMPAT, keep_volumes: bool = True, subgrid: bool = False, peaks=None,
                            uniqueness_ratio: float | None = None, propagation_ratio: float | None = None,
                            consistency_min_agree: int | None = None, consistency_tol: float | None = None, consistency_radius: int = 0,
                            u_dilation: int = 1, *, equalize_views=None, equalize_ref_view=None, equalize_joint=None,
                            equalize_max_gain: float = 4.0, level_dilation: int = 1, level_dilation_kind=DILATE_CUBIC,
                            derivative_channels: float = 0.0):
    """rslf_fine_to_coarse_run_host_lc / _u16_lc: the whole pyramid inside the library, host EPIs in (a list of V arrays
    [S,U] / [S,U,3]; float32, uint8 or uint16), host planes out.  Returns dict(out_map, out_valid [S,V,U], n_levels, stats)
    and, with want_levels, `levels`: per level dict(depth, valid, line_confidence, edge_confidence), each [S,V_p,U_p]
    (line_confidence is None in mode 0).

    keep=True: rslf_f2c_run_host -- the run stays on the device and a KeptFineToCoarse comes back; validity_rule
    (F2C_VALID_COMPAT, or F2C_VALID_REFERENCE for validity by C_d under par_use_disp_confidence_score) and keep_volumes apply
    to this form alone.

    subgrid (not in the reference): every level's sweep runs in the sub-grid mode (rslf_fine_to_coarse_run_host_sub,
    rslf_f2c_run_host_sub): the bounds of the coarser levels are tightened from off-grid disparities.

    peaks=True (not in the reference; keep=True only: rslf_f2c_run_host_pk): every level's sweep also runs in the peaks mode
    and the run keeps every level's peak planes and the fused peaks (KeptFineToCoarse.get_peaks / get_fused_peaks).
    uniqueness_ratio (None or 0: off; else in (0, 1], needs peaks=True): a level's valid pixels whose runner-up scores more
    than ratio * the winner's score become invalid, so a coarser level decides them.
    propagation_ratio (None or 0: off; else in (0, 1], needs keep=True and peaks=True; rslf_f2c_run_host_pr): every level's
    sweep withholds such pixels from propagation (Depth2DComputer); independent of uniqueness_ratio, both may be set.
    KeptFineToCoarse.propagation_ratio and .withheld(level) read it back.
    consistency_min_agree (not in the reference; None or 0: off; else m >= 1, needs keep=True and nothing else;
    rslf_f2c_run_host_cs): after a level's sweep, validity rule and uniqueness ratio, a pixel that is still valid becomes invalid
    unless agree >= min(seen, m) among the other views (view_consistency's counts; consistency_radius > 0: only views within
    it), so a coarser level decides it.  consistency_tol=None: one step of the hypothesis grid.
    KeptFineToCoarse.consistency_gate, .inconsistent(level) and .get_gate_counts(level) read it back.
    u_dilation: refused (require_no_u_dilation): the pyramid has no dilated levels; see level_dilation.
    derivative_channels (not in the reference's code, its report's second lead; 0 or None: off, today's call; else a finite
    weight w > 0; one-channel fields only; rslf_fine_to_coarse_run_host_dv, rslf_f2c_run_host_dv): the finest level becomes
    (x, min(|dx/du| * w / 2, hi), min(|dx/dv| * w / 2, hi)) on the device and the pyramid runs on it as on a three-channel
    field, bit for bit; a kept run describes itself with C = 3.
    level_dilation (not in the reference's code, its report's fourth lead; 1: off, today's call; else an integer factor in
    2..8, with level_dilation_kind a DILATE_*; rslf_fine_to_coarse_run_host_dl, rslf_f2c_run_host_dl): every level's SWEEP
    runs on the level's volume dilated along u with slope factor U_l / U_0 * factor, and its planes come back to the level's
    own grid before anything reads them: every result has the shapes it always had.  The level chain is untouched.  Not
    together with a line mode.  KeptFineToCoarse.level_dilation reads it back.
    equalize_views (not in the reference's code, the remedy its report names for global changes of illumination; None: off,
    today's call; else EQUALIZE_GAIN or EQUALIZE_AFFINE; rslf_fine_to_coarse_run_host_eq, rslf_f2c_run_host_eq): the finest
    level's upload is equalised per view on the device (Volume.equalized_views has the rule and equalize_ref_view,
    equalize_joint, equalize_max_gain), before the derivative channels, and the pyramid runs on it bit for bit as on the
    equalised field.  KeptFineToCoarse.equalize_views and .view_gains read it back."""
    require_no_u_dilation(u_dilation, "fine_to_coarse_run_host")
    eq = _equalize_mode(equalize_views, "fine_to_coarse_run_host")
    dl, dl_kind = _level_dilation(level_dilation, level_dilation_kind, "fine_to_coarse_run_host")
    require_no_line_confidence_level_dilated(line_mode, dl, "fine_to_coarse_run_host")
    dv = _derivative_weight(derivative_channels, "fine_to_coarse_run_host")
    want_cs = consistency_min_agree is not None and consistency_min_agree is not False and consistency_min_agree != 0
    cs_tol, cs_radius, cs_min_agree = 0.0, 0, 0
    if want_cs:
        if int(consistency_min_agree) < 0:
            raise ValueError("fine_to_coarse_run_host: consistency_min_agree %r is negative" % (consistency_min_agree,))
        if not keep:
            raise ValueError("fine_to_coarse_run_host: consistency_min_agree gates the validity of a kept run: pass keep=True")
        cs_tol, cs_radius, cs_min_agree = _consistency_args(
            grid_step(d_min, d_max, dim_d, "fine_to_coarse_run_host") if consistency_tol is None else consistency_tol,
            consistency_radius, consistency_min_agree, "fine_to_coarse_run_host: consistency_tol")
    want_peaks = peaks is not None and peaks is not False
    want_gate = _ratio_on(propagation_ratio)
    if want_gate and not keep:
        raise ValueError("fine_to_coarse_run_host: propagation_ratio reads the peaks planes of a kept run: pass keep=True, peaks=True")
    if want_gate and not want_peaks:
        raise ValueError("fine_to_coarse_run_host: propagation_ratio reads the peaks planes: pass peaks=True")
    gate = _propagation_ratio(propagation_ratio, "fine_to_coarse_run_host")
    want_ratio = uniqueness_ratio is not None and uniqueness_ratio != 0
    if not keep:
        if want_ratio:
            raise ValueError("fine_to_coarse_run_host: uniqueness_ratio reads the peaks planes of a kept run: pass keep=True, peaks=True")
        if want_peaks:   # the host-planes entries have a fixed set of level planes
            raise ValueError("fine_to_coarse_run_host: peaks is built for a kept run: pass keep=True (the host-planes form "
                             "hands out a fixed set of level planes)")
    if peaks is not None and not isinstance(peaks, (bool, np.bool_)):
        raise ValueError("fine_to_coarse_run_host: peaks is True or False (the kept run owns its peak planes)")
    if want_ratio and not want_peaks:
        raise ValueError("fine_to_coarse_run_host: uniqueness_ratio reads the peaks planes: pass peaks=True")
    if want_ratio and not 0.0 < float(uniqueness_ratio) <= 1.0:
        raise ValueError("fine_to_coarse_run_host: uniqueness_ratio %r is not in (0, 1]" % (uniqueness_ratio,))
    ctx = ctx or default_context()
    keep_alive, ptrs, dt, V, S, U, C_, stride = host_epis(epis, stride=True)
    if dv and C_ != 1:
        raise ValueError("fine_to_coarse_run_host: derivative_channels=%r needs a one-channel field, not C=%d" % (derivative_channels, C_))
    eq_args = (eq,) + (_equalize_args(S, C_, equalize_ref_view, equalize_joint, equalize_max_gain, "fine_to_coarse_run_host")
                       if eq else (0, 0, 4.0))
    L = _lib.lib()
    if keep:
        if want_levels:
            raise ValueError("fine_to_coarse_run_host: a kept run hands its levels out itself (KeptFineToCoarse.plane)")
        p, st, h = (parameters or Depth1DParameters()).to_c(), RslfStats(), C.c_void_p()
        ctx.use_current_stream()
        args = (ctx._h, ptrs, _ELEM[np.dtype(dt)], V, S, U, C_, stride, float(d_min), float(d_max), int(dim_d),
                float(epi_scale_factor), C.byref(p), int(max_pyr_depth), 1 if accept_all_last_scale else 0, int(line_mode),
                int(validity_rule), 1 if keep_volumes else 0, C.byref(h), C.byref(st))
        # the family's widest entry: what is off goes in neutral (0), and the run is the narrower entry's
        more = (1 if subgrid else 0, 1 if want_peaks else 0, float(uniqueness_ratio or 0.0), gate, cs_tol, cs_radius, cs_min_agree)
        if eq:
            check(L.rslf_f2c_run_host_eq(*args, *more, dv, dl, dl_kind, *eq_args), "rslf_f2c_run_host_eq")
        elif dl != 1:
            check(L.rslf_f2c_run_host_dl(*args, *more, dv, dl, dl_kind), "rslf_f2c_run_host_dl")
        elif dv:
            check(L.rslf_f2c_run_host_dv(*args, *more, dv), "rslf_f2c_run_host_dv")
        else:
            check(L.rslf_f2c_run_host_cs(*args, *more), "rslf_f2c_run_host_cs")
        return KeptFineToCoarse(h, ctx, st, (float(d_min), float(d_max), int(dim_d)))
    if validity_rule != F2C_VALID_COMPAT:
        raise ValueError("fine_to_coarse_run_host: validity_rule needs keep=True")
    out_map, out_valid = np.empty((S, V, U), np.float32), np.empty((S, V, U), np.uint8)
    p = (parameters or Depth1DParameters()).to_c()
    st, nl = RslfStats(), C.c_int()
    levels, lo = [], None
    if want_levels:
        check(L.rslf_f2c_pyramid_dims(V, U, int(max_pyr_depth), None, None, 0, C.byref(nl)), "rslf_f2c_pyramid_dims")
        P = nl.value
        Vp, Up = (C.c_int * P)(), (C.c_int * P)()
        check(L.rslf_f2c_pyramid_dims(V, U, int(max_pyr_depth), Vp, Up, P, C.byref(nl)), "rslf_f2c_pyramid_dims")
        for l in range(P):
            shape = (S, Vp[l], Up[l])
            levels.append(dict(depth=np.empty(shape, np.float32), valid=np.empty(shape, np.uint8),
                               line_confidence=np.empty(shape, np.float32) if line_mode != LINE_CONF_OFF else None,
                               edge_confidence=np.empty(shape, np.float32)))
        arr = lambda k: (C.c_void_p * P)(*[None if lv[k] is None else lv[k].ctypes.data for lv in levels])
        lo = _lib.RslfF2cLevelsOut(P, arr("depth"), arr("valid"), arr("line_confidence"), arr("edge_confidence"))
    rest = (V, S, U, C_, stride, float(d_min), float(d_max), int(dim_d), float(epi_scale_factor), C.byref(p), int(max_pyr_depth),
            1 if accept_all_last_scale else 0, out_map.ctypes.data_as(C.c_void_p), out_valid.ctypes.data_as(C.c_void_p),
            C.byref(nl), C.byref(st), int(line_mode), C.byref(lo) if lo is not None else None)
    ctx.use_current_stream()
    # the family's widest entry, which takes any element type
    if eq:
        check(L.rslf_fine_to_coarse_run_host_eq(ctx._h, ptrs, _ELEM[np.dtype(dt)], *rest, 1 if subgrid else 0, dv, dl, dl_kind, *eq_args),
              "rslf_fine_to_coarse_run_host_eq")
    elif dl != 1:
        check(L.rslf_fine_to_coarse_run_host_dl(ctx._h, ptrs, _ELEM[np.dtype(dt)], *rest, 1 if subgrid else 0, dv, dl, dl_kind),
              "rslf_fine_to_coarse_run_host_dl")
    elif dv:
        check(L.rslf_fine_to_coarse_run_host_dv(ctx._h, ptrs, _ELEM[np.dtype(dt)], *rest, 1 if subgrid else 0, dv),
              "rslf_fine_to_coarse_run_host_dv")
    else:
        check(L.rslf_fine_to_coarse_run_host_sub(ctx._h, ptrs, _ELEM[np.dtype(dt)], *rest, 1 if subgrid else 0),
              "rslf_fine_to_coarse_run_host_sub")
    out = dict(out_map=out_map, out_valid=out_valid, n_levels=int(nl.value), stats=st)
    if want_levels:
        out["levels"] = levels
    return out


class FineToCoarse:
    """rslf::FineToCoarse<T> (include/rslf_fine_to_coarse.hpp:26-81, :103-324): a pyramid of Depth2DComputers,
    each level halving (v, u) -- never s --, with slope_factor = U_p / U_0, per-pixel hypothesis ranges
    tightened from the finer level, and a coarse-to-fine fusion of the disparity maps.

    `epis`: the reference's Vec<Mat> (list of V arrays [S,U] / [S,U,3]) or a dense array [V,S,U(,C)],
    float32, uint8 or uint16.  An integer light field keeps its own arithmetic through the pyramid, as the reference's
    CV_8U / CV_16U Mats do.

    `line_confidence_mode` (None, 0, 1 or 2) is the -D_USE_LINE_CONFIDENCE_SCORE build of the pyramid: every level's
    computer runs in that mode with a C_l plane of its own, and in mode 2 (without par_use_disp_confidence_score) each
    level's validity -- the next level's bounds and the fusion -- is C_l > par_line_score_threshold (dc.hpp:903-904).
    None is the default build; parameters whose par_line_confidence_mode is set are then refused.

    `derivative_channels` (not in the reference's code, its report's second lead; 0 or None: off; else a finite weight w > 0,
    one-channel fields only): the raw finest level becomes (x, min(|dx/du| * w / 2, hi), min(|dx/dv| * w / 2, hi)) on the
    device (derivative_channels(), once, on f2c_input's output) and the loop runs on it as on any three-channel field.

    `level_dilation` / `level_dilation_kind` (not in the reference's code, its report's fourth lead; 1: off; else a factor in
    2..8 and a DILATE_*): run() sweeps every level on its volume dilated along u (Volume.dilated_u) with the slope factor
    times the factor and the level's ranges by dilate_ranges_u, and writes the columns u * factor of the sweep's planes into
    the level's computer: the computers and every getter keep answering on the level's own grid.  Not with a line mode.

    `equalize_views` (not in the reference's code, the remedy its report names for global changes of illumination; None:
    off; else EQUALIZE_GAIN or EQUALIZE_AFFINE, with `equalize_ref_view`, `equalize_joint`, `equalize_max_gain` as
    Volume.equalized_views takes them): the raw finest level is equalised per view on the device (equalize_views(), once,
    in place, on f2c_input's output, before the derivative channels); .m_view_gains holds the [S, C, 2] coefficients."""

    def __init__(self, epis, d_min: float, d_max: float, dim_d: int, epi_scale_factor: float = -1.0,
                 parameters: Depth1DParameters | None = None, max_pyr_depth: int = -1, accept_all_last_scale: bool = True,
                 ctx: Context | None = None, line_confidence_mode: int | None = None, subgrid: bool = False, peaks=None,
                 propagation_ratio=None, consistency_min_agree=None, u_dilation: int = 1, *, equalize_views=None,
                 equalize_ref_view=None, equalize_joint=None, equalize_max_gain: float = 4.0, level_dilation: int = 1,
                 level_dilation_kind=DILATE_CUBIC, derivative_channels: float = 0.0):
        self.m_level_dilation, self.m_level_dilation_kind = _level_dilation(level_dilation, level_dilation_kind, "FineToCoarse")
        # not in the reference: the finest level's upload equalised per view (K19); 0: off
        self.m_equalize_views = _equalize_mode(equalize_views, "FineToCoarse")
        self.m_view_gains = None
        # not in the reference: a one-channel field goes down the pyramid as (x, |dx/du|, |dx/dv|) by this weight (K17); 0: off
        self.m_derivative_channels = _derivative_weight(derivative_channels, "FineToCoarse")
        require_no_peaks(peaks, "FineToCoarse")   # (the pyramid's levels carry no peak planes)
        require_no_u_dilation(u_dilation, "FineToCoarse")   # (nor dilated levels)
        require_no_propagation_ratio(propagation_ratio, "FineToCoarse")
        require_no_consistency_gate(consistency_min_agree, "FineToCoarse")
        self.m_parameters = parameters or Depth1DParameters.get_default()
        self.m_subgrid = bool(subgrid)   # not in the reference: every level's sweep in the sub-grid mode (Depth2DComputer)
        f2c_line_mode(self.m_parameters, line_confidence_mode, "FineToCoarse")
        require_no_line_confidence_level_dilated(line_confidence_mode if line_confidence_mode is not None
                                                 else self.m_parameters.par_line_confidence_mode, self.m_level_dilation, "FineToCoarse")
        ctx = ctx or default_context()
        self.m_computers: list[Depth2DComputer] = []
        self.m_parameter_instances: list[Depth1DParameters] = []
        raw0, dt = f2c_input(epis, ctx)
        if self.m_equalize_views:   # once, in place, on the finest level; everything below reads the equalised intensity
            raw0, self.m_view_gains = _equalize_views_dense(ctx, raw0, self.m_equalize_views, equalize_ref_view, equalize_joint,
                                                            equalize_max_gain, dt, inplace=True)
        if self.m_derivative_channels:   # once, on the finest level; the features go down with the intensity
            if raw0.shape[3] != 1:
                raise ValueError("FineToCoarse: derivative_channels=%r needs a one-channel field, not C=%d"
                                 % (derivative_channels, raw0.shape[3]))
            raw0 = _derivative_channels_dense(ctx, raw0, self.m_derivative_channels, dt)
        for _, _, par, scale, raw in f2c_pyramid(raw0, dt, epi_scale_factor, self.m_parameters, max_pyr_depth, ctx, line_confidence_mode):
            vol = Volume.from_dense(raw, scale, ctx)
            self.m_computers.append(Depth2DComputer(vol, d_min, d_max, dim_d, parameters=par, subgrid=self.m_subgrid))
            self.m_parameter_instances.append(par)
        if accept_all_last_scale:
            self.m_computers[-1].set_accept_all(True)                                              # f2c.hpp:157-158
        self._dmin, self._dmax = float(d_min), float(d_max)

    def run(self) -> None:
        """f2c.hpp:171-299."""
        for p, comp in enumerate(self.m_computers):
            if self.m_level_dilation != 1:
                self._run_level_dilated(p, comp)
                continue
            if p == 0:
                comp.run(want_stats=True)
                continue
            vol, up = comp.m_epis, self.m_computers[p - 1]
            dmin, dmax = f2c_ranges(vol.ctx, up.m_best_depth_s_v_u, up.get_valid_depths_mask_s_v_u(), vol.V, vol.U, self._dmin, self._dmax)
            comp.m_dmin_s_v_u, comp.m_dmax_s_v_u = dmin, dmax
            # Depth2DComputer::run with per-pixel ranges (edit_dmin / edit_dmax, dc.hpp:201-203)
            for t in (comp.m_edge_confidence_s_v_u, comp.m_disp_confidence_s_v_u, comp.m_best_depth_s_v_u, comp.m_rbar_s_v_u,
                      comp.m_line_confidence_s_v_u):
                if t is not None:
                    t.zero_()
            comp.m_edge_confidence_mask_s_v_u = compute_2D_edge_confidence(vol, comp.m_edge_confidence_s_v_u, comp.m_parameters)
            comp.stats = compute_2D_depth_epi(vol, dmin, dmax, comp.m_dim_d, comp.m_edge_confidence_s_v_u,
                                              comp.m_edge_confidence_mask_s_v_u, comp.m_disp_confidence_s_v_u,
                                              comp.m_best_depth_s_v_u, comp.m_rbar_s_v_u, comp.m_parameters,
                                              scan_mask_s_v_u=comp.m_scan_mask_s_v_u, want_stats=True,
                                              a_line_confidence_s_v_u=comp.m_line_confidence_s_v_u, subgrid=self.m_subgrid)

    def _run_level_dilated(self, p: int, comp: "Depth2DComputer") -> None:
        """Level p's sweep in the frame dilated along u: a computer of its own on comp's volume (Volume.dilated_u, the slope
        factor times the factor), the level's ranges by dilate_ranges_u, and the columns u * factor of its planes into comp."""
        f, vol = self.m_level_dilation, comp.m_epis
        dil = Depth2DComputer(vol, self._dmin, self._dmax, comp.m_dim_d, parameters=comp.m_parameters, subgrid=self.m_subgrid,
                              u_dilation=f, dilation_kind=self.m_level_dilation_kind)
        if p == 0:
            dil.run(want_stats=True)
        else:
            up = self.m_computers[p - 1]
            dmin, dmax = f2c_ranges(vol.ctx, up.m_best_depth_s_v_u, up.get_valid_depths_mask_s_v_u(), vol.V, vol.U, self._dmin, self._dmax)
            comp.m_dmin_s_v_u, comp.m_dmax_s_v_u = dmin, dmax
            dmin_d, dmax_d = dilate_ranges_u(vol.ctx, dmin, dmax, f)
            for t in (dil.m_edge_confidence_s_v_u, dil.m_disp_confidence_s_v_u, dil.m_best_depth_s_v_u, dil.m_rbar_s_v_u):
                t.zero_()
            dil.m_edge_confidence_mask_s_v_u = compute_2D_edge_confidence(dil.m_epis, dil.m_edge_confidence_s_v_u, dil.m_parameters)
            dil.stats = compute_2D_depth_epi(dil.m_epis, dmin_d, dmax_d, dil.m_dim_d, dil.m_edge_confidence_s_v_u,
                                             dil.m_edge_confidence_mask_s_v_u, dil.m_disp_confidence_s_v_u, dil.m_best_depth_s_v_u,
                                             dil.m_rbar_s_v_u, dil.m_parameters, scan_mask_s_v_u=dil.m_scan_mask_s_v_u,
                                             want_stats=True, subgrid=self.m_subgrid)
        (comp.m_best_depth_s_v_u, comp.m_edge_confidence_s_v_u, comp.m_disp_confidence_s_v_u, comp.m_edge_confidence_mask_s_v_u,
         comp.m_scan_mask_s_v_u) = undilate_many_u(vol.ctx, [dil.m_best_depth_s_v_u, dil.m_edge_confidence_s_v_u,
                                                             dil.m_disp_confidence_s_v_u, dil.m_edge_confidence_mask_s_v_u,
                                                             dil.m_scan_mask_s_v_u], f)
        comp.m_rbar_s_v_u = dil.undilated("rbar")
        comp.stats = dil.stats   # (what the sweep did, in the dilated frame)

    def get_results(self):
        """f2c.hpp:302-324 -> (out_map_s_v_u [S,V,U] f32, out_validity_s_v_u [S,V,U] u8) at the finest scale."""
        comps = self.m_computers
        return f2c_fuse(comps[0].m_epis.ctx, [c.m_best_depth_s_v_u.contiguous() for c in comps],
                        [c.get_valid_depths_mask_s_v_u().contiguous() for c in comps])

    def get_consistency(self, *args, **kwargs):
        no_consistency("FineToCoarse (the Python level loop)")

    def get_warped_views(self, *args, **kwargs):
        no_view_warp("FineToCoarse (the Python level loop)")

    def get_view_prediction(self, *args, **kwargs):
        no_view_warp("FineToCoarse (the Python level loop)", "get_view_prediction")

    def get_novel_views(self, *args, **kwargs):
        no_novel_view("FineToCoarse (the Python level loop)")

    def get_novel_view_prediction(self, *args, **kwargs):
        no_novel_view("FineToCoarse (the Python level loop)", "get_novel_view_prediction")

    def _fit_mode(self, saturate: bool) -> int:
        return FIT_QUANTILE if saturate else FIT_MEANSTD   # ImageConverter_uchar::fit(img, saturate), rslf_plot.cpp:65-98

    def _shadow_volume(self, level: int):
        """The volume and level of the getters' shadow cut (f2c.hpp:360-372, :466-481), or (None, 0) without
        par_cut_shadows.  The reference compares against _SHADOW_NORMALIZED_LEVEL; here it is par_shadow_level, whose
        default is that constant."""
        if not self.m_parameters.par_cut_shadows:
            return None, 0.0
        return self.m_computers[level].m_epis, float(self.m_parameters.par_shadow_level)

    def get_coloured_depth_maps(self, lut_bgr=None, saturate: bool = True) -> torch.Tensor:
        """f2c.hpp:325-378: the fused disparities of every view through ONE converter, fitted on the fused plane
        (int)std::round(S / 2.0) (saturate: 2 % / 98 % quantiles, else min and mean + 12 std), colour-mapped, black where the
        fused validity is 0 and, with par_cut_shadows, where the finest level's radiance is in shadow -> [S, V, U, 3] uint8
        BGR.  S = 1 raises ValueError: the reference's index is then S itself.  NaN disparities: unspecified."""
        ctx = self.m_computers[0].m_epis.ctx
        mid = _index_rule("rslf_render_centre_index", self.m_computers[0].m_epis.S)
        out_map, out_valid = self.get_results()
        lo, hi = render_fit(ctx, out_map[mid], None, self._fit_mode(saturate))
        vol, level = self._shadow_volume(0)
        return render_planes(ctx, out_map, lo, hi, RENDER_AFFINE, lut_bgr, out_valid, MASK_BLACK, vol, SLICE_VIEW, 0, level)

    def get_coloured_depth_pyr(self, s: int = -1, lut_bgr=None, saturate: bool = True) -> list:
        """f2c.hpp:491-519: view s (-1: (int)std::round(S / 2.0)) of every level, finest first, through the converter fitted
        on level 0's plane before any masking; black outside each level's validity; no shadow cut -> a list of
        [V_p, U_p, 3] uint8 BGR.  ValueError where the reference's index runs off the end (S = 1)."""
        comps = self.m_computers
        S = comps[0].m_epis.S
        s = _index_rule("rslf_render_centre_index", S) if s == -1 else int(s)
        if not 0 <= s < S:
            raise ValueError("view %d of %d" % (s, S))
        out, lo, hi = [], 0.0, 0.0
        for p, comp in enumerate(comps):
            ctx, plane = comp.m_epis.ctx, comp.m_best_depth_s_v_u[s]
            if p == 0:
                lo, hi = render_fit(ctx, plane, None, self._fit_mode(saturate))
            valid = comp.get_valid_depths_mask_s_v_u()[s]
            out.append(render_planes(ctx, plane.unsqueeze(0), lo, hi, RENDER_AFFINE, lut_bgr, valid.unsqueeze(0), MASK_BLACK)[0])
        return out

    def get_coloured_epi_pyr(self, v: int = -1, lut_bgr=None, saturate: bool = True) -> list:
        """f2c.hpp:432-488: the S x U_p slice of every level at scanline (int)std::round(1.0 * v * V_p / V_0) (v = -1:
        (int)std::round(V_0 / 2.0)), finest first.  Invalid pixels count as 0 in the fit (level 0 only) and in the render, so
        they get the colour of level(0), not black; then, with par_cut_shadows, the shadow cut against the level's own
        volume -> a list of [S, U_p, 3] uint8 BGR.  ValueError where the reference's row index reaches V_p (V_0 = 1, or
        v = V_0 - 1 with V_p = V_0 / 2)."""
        comps = self.m_computers
        V0 = comps[0].m_epis.V
        v = _index_rule("rslf_render_centre_index", V0) if v == -1 else int(v)
        out, lo, hi = [], 0.0, 0.0
        for p, comp in enumerate(comps):
            ctx = comp.m_epis.ctx
            row = _index_rule("rslf_render_scaled_row", v, comp.m_epis.V, V0)
            plane, valid = comp.m_best_depth_s_v_u[:, row, :], comp.get_valid_depths_mask_s_v_u()[:, row, :]
            if p == 0:
                lo, hi = render_fit(ctx, plane, valid, self._fit_mode(saturate))
            vol, level = self._shadow_volume(p)
            out.append(render_planes(ctx, plane.unsqueeze(0), lo, hi, RENDER_AFFINE, lut_bgr, valid.unsqueeze(0), MASK_ZERO_VALUE,
                                     vol, SLICE_EPI, row, level)[0])
        return out
