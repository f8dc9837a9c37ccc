"""ctypes binding of include/rslf_hip.h (librslf_hip.so).

There is no fallback: if the library is missing or fails to load, or no gfx950
device is visible when a context is created, this raises.
"""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build

_LIB = None

ABI_VERSION = 6

# every symbol include/rslf_hip.h declares
SYMBOLS = [
    "rslf_abi_version", "rslf_status_string", "rslf_last_error", "rslf_device_count", "rslf_default_params",
    "rslf_ctx_create", "rslf_ctx_destroy", "rslf_ctx_set_stream", "rslf_ctx_synchronize", "rslf_ctx_set_debug", "rslf_debug_inject",
    "rslf_multi_create", "rslf_multi_destroy", "rslf_multi_device_count", "rslf_multi_set_chunk_rows", "rslf_multi_peer_access",
    "rslf_multi_depth1d_pile_f32", "rslf_multi_depth1d_pile_u8", "rslf_multi_depth1d_pile_f32_dev",
    "rslf_multi_depth2d_run_f32", "rslf_multi_depth2d_run_u8", "rslf_multi_fine_to_coarse_run_host",
    "rslf_volume_create", "rslf_volume_destroy", "rslf_volume_describe",
    "rslf_volume_upload_epis_f32", "rslf_volume_upload_epis_u8",
    "rslf_volume_upload_images_f32", "rslf_volume_upload_images_u8", "rslf_volume_pack_device_f32",
    "rslf_edge_confidence_pile", "rslf_depth_epi_pile", "rslf_selective_median",
    "rslf_depth1d_pile_run", "rslf_depth1d_pile_run_host", "rslf_last_scan_kernel_ms", "rslf_scan_time_total_ms", "rslf_last_scan_row_exact",
    "rslf_edge_confidence_2d", "rslf_depth_epi_2d", "rslf_depth2d_run",
    "rslf_sweep_begin", "rslf_sweep_visit_scan", "rslf_sweep_visit_finish", "rslf_sweep_end",
    "rslf_depth_epi_scan", "rslf_depth1d_run",
    "rslf_f2c_level_dims", "rslf_downsample_epis_f32", "rslf_downsample_epis_u8", "rslf_device_max_f32", "rslf_f2c_tighten_bounds", "rslf_f2c_fuse",
    "rslf_depth2d_run_host", "rslf_fine_to_coarse_run_host", "rslf_kernel_columns_pile", "rslf_volume_upload_images_xf_f32", "rslf_volume_upload_images_xf_u8",
    # CV_16U light fields
    "rslf_volume_upload_epis_u16", "rslf_volume_upload_images_u16", "rslf_volume_upload_images_xf_u16", "rslf_downsample_epis_u16",
    "rslf_multi_depth1d_pile_u16", "rslf_multi_depth2d_run_u16", "rslf_fine_to_coarse_run_host_u16",
    "rslf_multi_fine_to_coarse_run_host_u16",
    # rendering (K6)
    "rslf_render_fit", "rslf_render_planes", "rslf_render_epi_lines", "rslf_render_centre_index", "rslf_render_scaled_row",
    "rslf_render_fit_many", "rslf_render_planes_each", "rslf_render_planes_host", "rslf_render_epi_lines_host",
    # line confidence of the 2-D sweep (K7)
    "rslf_line_confidence_pile", "rslf_sweep_line_confidence", "rslf_depth_epi_2d_lc", "rslf_depth2d_run_lc", "rslf_depth2d_run_host_lc",
    # fine-to-coarse with the line confidence
    "rslf_f2c_pyramid_dims", "rslf_fine_to_coarse_run_host_lc", "rslf_fine_to_coarse_run_host_u16_lc",
    # fine-to-coarse kept on the device
    "rslf_f2c_run_host", "rslf_f2c_run_destroy", "rslf_f2c_run_describe", "rslf_f2c_run_copy", "rslf_f2c_run_volume",
    "rslf_f2c_run_render_depth_maps", "rslf_f2c_run_render_depth_maps_host", "rslf_f2c_run_render_depth_pyr",
    "rslf_f2c_run_render_depth_pyr_host", "rslf_f2c_run_render_epi_pyr", "rslf_f2c_run_render_epi_pyr_host",
    # the scan's score matrix
    "rslf_depth_epi_scores", "rslf_depth_epi_scores_host",
    # ... and its peaks
    "rslf_score_peaks", "rslf_depth_epi_peaks", "rslf_depth_epi_peaks_host",
    # sub-grid disparities in the pile step (K9)
    "rslf_subgrid_refine", "rslf_depth_epi_pile_sub", "rslf_depth_epi_scan_sub", "rslf_depth1d_run_sub", "rslf_depth1d_pile_run_sub",
    "rslf_depth1d_pile_run_host_sub",
    # ... in the 2-D sweep and fine-to-coarse
    "rslf_sweep_subgrid", "rslf_depth_epi_2d_sub", "rslf_depth2d_run_sub", "rslf_depth2d_run_host_sub",
    "rslf_fine_to_coarse_run_host_sub", "rslf_f2c_run_host_sub", "rslf_f2c_run_subgrid",
    # runner-up peaks in the 2-D sweep (K10)
    "rslf_sweep_peaks", "rslf_depth_epi_2d_pk", "rslf_depth2d_run_pk", "rslf_depth2d_run_host_pk",
    # a kept fine-to-coarse run's peaks per level and validity by uniqueness (K11)
    "rslf_f2c_run_host_pk", "rslf_f2c_run_peaks", "rslf_f2c_run_uniqueness", "rslf_f2c_unique_mask", "rslf_f2c_fuse_peaks",
    # the sweep gate: ambiguous pixels withheld from propagation by peak ratio
    "rslf_sweep_propagation_ratio", "rslf_sweep_withheld", "rslf_depth_epi_2d_pr", "rslf_depth2d_run_pr", "rslf_depth2d_run_host_pr",
    "rslf_f2c_run_host_pr", "rslf_f2c_run_propagation_ratio", "rslf_f2c_run_withheld",
    # cross-view consistency of a sweep's disparity planes (K12)
    "rslf_view_consistency", "rslf_view_consistency_host", "rslf_f2c_run_consistency", "rslf_f2c_run_consistency_host",
    # a kept fine-to-coarse run's validity by cross-view consistency (K13)
    "rslf_f2c_run_host_cs", "rslf_f2c_run_consistency_gate", "rslf_f2c_run_inconsistent", "rslf_f2c_consistency_mask",
    # the view warp: any view position from a sweep's planes, z-buffered (K14)
    "rslf_view_warp", "rslf_view_warp_host", "rslf_f2c_run_view_warp", "rslf_f2c_run_view_warp_host",
    # the novel view: the warp's holes filled, the views that see a point blended (K15)
    "rslf_novel_view", "rslf_novel_view_host", "rslf_f2c_run_novel_view", "rslf_f2c_run_novel_view_host",
    # the dilation along u and the way back (K16)
    "rslf_dilated_width", "rslf_volume_dilate_u", "rslf_planes_undilate_u", "rslf_planes_undilate_u_host",
    # the derivative channels: a one-channel field as (x, |dx/du|, |dx/dv|), and the pyramid on it (K17)
    "rslf_volume_derivative_channels", "rslf_derivative_channels_dense", "rslf_fine_to_coarse_run_host_dv", "rslf_f2c_run_host_dv",
    # the level dilation: every level's sweep of the pyramid on EPIs dilated along u (K18)
    "rslf_planes_dilate_ranges_u", "rslf_planes_dilate_ranges_u_host", "rslf_planes_undilate_many_u", "rslf_fine_to_coarse_run_host_dl",
    "rslf_f2c_run_host_dl", "rslf_f2c_run_level_dilation",
    # the per-view equalisation: a view's quantised statistics, (a, b) per view and channel, and the pyramid on it (K19)
    "rslf_volume_view_stats", "rslf_view_stats_dense", "rslf_equalize_coefficients", "rslf_volume_equalize_views",
    "rslf_volume_apply_view_gains", "rslf_equalize_views_dense", "rslf_fine_to_coarse_run_host_eq", "rslf_f2c_run_host_eq",
    "rslf_f2c_run_equalize", "rslf_apply_view_gains_dense", "rslf_f2c_run_view_gains_channels",
]


class RslfParams(C.Structure):
    """rslf_params == rslf::Depth1DParameters<T> (core.hpp:66-142)."""

    _fields_ = [
        ("edge_score_threshold", C.c_float),
        ("line_score_threshold", C.c_float),
        ("disp_score_threshold", C.c_float),
        ("raw_score_threshold", C.c_float),
        ("mean_shift_max_iter", C.c_float),
        ("edge_confidence_filter_size", C.c_int),
        ("edge_confidence_opening_type", C.c_int),
        ("edge_confidence_opening_size", C.c_int),
        ("median_filter_size", C.c_int),
        ("median_filter_epsilon", C.c_float),
        ("propagation_epsilon", C.c_float),
        ("slope_factor", C.c_float),
        ("cut_shadows", C.c_int),
        ("shadow_level", C.c_float),
        ("kernel_bandwidth", C.c_float),
        ("interpolation", C.c_int),
        ("use_disp_confidence_score", C.c_int),
    ]


class RslfVolumeDesc(C.Structure):
    _fields_ = [
        ("V", C.c_int), ("S", C.c_int), ("U", C.c_int), ("C", C.c_int),
        ("pitch", C.c_int),
        ("d_base", C.c_void_p),
        ("bytes", C.c_size_t),
        ("min_value", C.c_float),
        ("max_value", C.c_float),
    ]


class RslfStats(C.Structure):
    _fields_ = [
        ("pixels_scanned", C.c_int64),
        ("units", C.c_int64),
        ("scan_kernel", C.c_int),
        ("s_pad", C.c_int),
    ]


class RslfPeaks(C.Structure):
    """rslf_peaks: the five planes of the score-row peaks, device or host pointers, each nullable."""

    _fields_ = [
        ("idx", C.c_void_p), ("score", C.c_void_p), ("disp", C.c_void_p), ("runner_idx", C.c_void_p), ("runner_score", C.c_void_p),
    ]


class RslfViewCounts(C.Structure):
    """rslf_view_counts: the four count planes of the cross-view consistency check, int32 [S][V][U], each nullable."""

    _fields_ = [("seen", C.c_void_p), ("agree", C.c_void_p), ("above", C.c_void_p), ("below", C.c_void_p)]


class RslfViewWarpOut(C.Structure):
    """rslf_view_warp_out: the nine planes of the view warp, device or host pointers, each nullable."""

    _fields_ = [("hit", C.c_void_p), ("depth", C.c_void_p), ("src_view", C.c_void_p), ("src_col", C.c_void_p), ("count", C.c_void_p),
                ("colour", C.c_void_p), ("err", C.c_void_p), ("row_err", C.c_void_p), ("row_hits", C.c_void_p)]


class RslfNovelViewParams(C.Structure):
    """rslf_novel_view_params."""

    _fields_ = [("radius", C.c_int), ("nearer", C.c_int), ("max_gap", C.c_int), ("sources", C.c_int), ("tol", C.c_float)]


class RslfNovelViewOut(C.Structure):
    """rslf_novel_view_out: the seven planes of the novel view, device or host pointers, each nullable."""

    _fields_ = [("colour", C.c_void_p), ("depth", C.c_void_p), ("fill", C.c_void_p), ("n_src", C.c_void_p), ("err", C.c_void_p),
                ("row_err", C.c_void_p), ("row_cov", C.c_void_p)]


class RslfF2cLevelsOut(C.Structure):
    """rslf_f2c_levels_out: per level, host pointers for the planes the caller wants."""

    _fields_ = [
        ("capacity", C.c_int),
        ("h_depth_svu", C.POINTER(C.c_void_p)),
        ("h_valid_svu", C.POINTER(C.c_void_p)),
        ("h_Cl_svu", C.POINTER(C.c_void_p)),
        ("h_Ce_svu", C.POINTER(C.c_void_p)),
    ]


F2C_MAX_LEVELS = 32   # RSLF_F2C_MAX_LEVELS


class RslfF2cRunDesc(C.Structure):
    """rslf_f2c_run_desc: what a kept fine-to-coarse run holds."""

    _fields_ = [
        ("n_levels", C.c_int), ("S", C.c_int), ("C", C.c_int), ("device", C.c_int), ("elem", C.c_int), ("line_mode", C.c_int),
        ("validity_rule", C.c_int), ("keep_volumes", C.c_int), ("planes_held", C.c_uint),
        ("V", C.c_int * F2C_MAX_LEVELS), ("U", C.c_int * F2C_MAX_LEVELS), ("epi_scale_factor", C.c_float * F2C_MAX_LEVELS),
        ("device_bytes", C.c_size_t),
    ]


class RslfError(RuntimeError):
    def __init__(self, status: int, where: str):
        L = lib()
        msg = L.rslf_last_error().decode(errors="replace")
        what = L.rslf_status_string(status).decode()
        super().__init__("%s: %s (%d): %s" % (where, what, status, msg))
        self.status = status


def library_path() -> str:
    # RSLF_LIBRARY: load another build of the same ABI (A/B timing of kernel variants)
    return os.environ.get("RSLF_LIBRARY") or _build.SO


def lib():
    """Load librslf_hip.so (building it first if hipcc is at hand and it is stale)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # torch first: it brings its own copy of the HIP runtime (same soname as /opt/rocm's), and a process must not end up
    # with the library bound to one copy and torch to the other -- whichever loads first serves both, and with ours
    # first torch's streams and tensors and the library's context no longer see the same devices
    import torch  # noqa: F401
    path = library_path()
    if not os.path.exists(path):
        try:
            _build.build()
        except Exception as e:  # noqa: BLE001
            raise RuntimeError(
                "librslf_hip.so is missing and could not be built (%s). The HIP library IS the product: "
                "there is no CPU fallback. Run `python -m remotesensingproject_amd.build`." % e) from e
    L = C.CDLL(path)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    L.rslf_abi_version.restype = ci
    L.rslf_status_string.restype = C.c_char_p
    L.rslf_status_string.argtypes = [ci]
    L.rslf_last_error.restype = C.c_char_p
    L.rslf_device_count.restype = ci
    L.rslf_default_params.restype = None
    L.rslf_default_params.argtypes = [C.POINTER(RslfParams)]
    L.rslf_ctx_create.argtypes = [ci, C.POINTER(vp)]
    L.rslf_ctx_destroy.argtypes = [vp]
    L.rslf_ctx_set_stream.argtypes = [vp, vp]
    L.rslf_ctx_set_debug.argtypes = [vp, C.c_char_p, C.c_int]
    L.rslf_ctx_synchronize.argtypes = [vp]
    L.rslf_volume_create.argtypes = [vp, ci, ci, ci, ci, C.POINTER(vp)]
    L.rslf_volume_destroy.argtypes = [vp]
    L.rslf_volume_describe.argtypes = [vp, C.POINTER(RslfVolumeDesc)]
    L.rslf_volume_upload_epis_f32.argtypes = [vp, C.POINTER(vp), C.c_size_t, cf, C.POINTER(cf)]
    L.rslf_volume_upload_epis_u8.argtypes = [vp, C.POINTER(vp), C.c_size_t]
    L.rslf_volume_upload_images_f32.argtypes = [vp, C.POINTER(vp), C.c_size_t, cf, C.POINTER(cf)]
    L.rslf_volume_upload_images_u8.argtypes = [vp, C.POINTER(vp), C.c_size_t]
    L.rslf_volume_upload_images_xf_f32.argtypes = [vp, C.POINTER(vp), C.c_size_t, cf, C.POINTER(cf), ci, ci]
    L.rslf_volume_upload_images_xf_u8.argtypes = [vp, C.POINTER(vp), C.c_size_t, ci, ci]
    L.rslf_volume_upload_epis_u16.argtypes = L.rslf_volume_upload_epis_f32.argtypes
    L.rslf_volume_upload_images_u16.argtypes = L.rslf_volume_upload_images_f32.argtypes
    L.rslf_volume_upload_images_xf_u16.argtypes = L.rslf_volume_upload_images_xf_f32.argtypes
    L.rslf_volume_pack_device_f32.argtypes = [vp, vp, cf, C.POINTER(cf)]
    L.rslf_edge_confidence_pile.argtypes = [vp, vp, ci, C.POINTER(RslfParams), vp, vp]
    L.rslf_depth_epi_pile.argtypes = [vp, vp, vp, vp, cf, cf, ci, ci, vp, vp, vp, vp, vp, C.POINTER(RslfParams),
                                      vp, vp, vp, vp, C.POINTER(RslfStats)]
    L.rslf_selective_median.argtypes = [vp, vp, vp, vp, ci, ci, vp, cf]
    L.rslf_depth_epi_scan.argtypes = [vp, vp, vp, vp, cf, cf, ci, ci, vp, vp, vp, vp, vp, C.POINTER(RslfParams),
                                      vp, vp, vp, C.POINTER(RslfStats)]
    L.rslf_depth_epi_scores.argtypes = [vp, vp, vp, vp, cf, cf, ci, ci, C.POINTER(RslfParams), vp, ci, ci, vp, C.POINTER(RslfStats)]
    L.rslf_depth_epi_scores_host.argtypes = L.rslf_depth_epi_scores.argtypes
    L.rslf_score_peaks.argtypes = [vp, vp, ci, ci, vp, vp, cf, cf, vp, ci, ci, C.POINTER(RslfPeaks)]
    L.rslf_depth_epi_peaks.argtypes = [vp, vp, vp, vp, cf, cf, ci, ci, C.POINTER(RslfParams), vp, ci, ci, C.POINTER(RslfPeaks),
                                       C.POINTER(RslfStats)]
    L.rslf_depth_epi_peaks_host.argtypes = L.rslf_depth_epi_peaks.argtypes
    L.rslf_depth1d_run.argtypes = [vp, vp, cf, cf, ci, ci, C.POINTER(RslfParams), vp, vp, vp, vp, vp, vp, vp,
                                   C.POINTER(RslfStats)]
    L.rslf_depth1d_pile_run.argtypes = [vp, vp, cf, cf, ci, ci, C.POINTER(RslfParams), vp, vp, vp, vp, vp, vp, vp, vp,
                                        C.POINTER(RslfStats)]
    L.rslf_depth1d_pile_run_host.argtypes = L.rslf_depth1d_pile_run.argtypes
    L.rslf_subgrid_refine.argtypes = [vp, vp, vp, vp, cf, cf, ci, ci, C.POINTER(RslfParams), vp, vp, vp, vp, vp]
    L.rslf_depth_epi_pile_sub.argtypes = L.rslf_depth_epi_pile.argtypes + [ci]
    L.rslf_depth_epi_scan_sub.argtypes = L.rslf_depth_epi_scan.argtypes + [ci]
    L.rslf_depth1d_run_sub.argtypes = L.rslf_depth1d_run.argtypes + [ci]
    L.rslf_depth1d_pile_run_sub.argtypes = L.rslf_depth1d_pile_run.argtypes + [ci]
    L.rslf_depth1d_pile_run_host_sub.argtypes = L.rslf_depth1d_pile_run.argtypes + [ci]
    L.rslf_last_scan_kernel_ms.argtypes = [vp, C.POINTER(cf)]
    L.rslf_scan_time_total_ms.argtypes = [vp, C.POINTER(cf), C.POINTER(ci)]
    L.rslf_last_scan_row_exact.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
    L.rslf_sweep_begin.argtypes = [vp, vp, vp, vp, ci, ci, ci]
    L.rslf_sweep_visit_scan.argtypes = [vp, vp, vp, vp, cf, cf, ci, ci, vp, vp, vp, vp, vp, C.POINTER(RslfParams)]
    L.rslf_sweep_visit_finish.argtypes = [vp, vp, ci, vp, vp, vp, vp, C.POINTER(RslfParams)]
    L.rslf_sweep_end.argtypes = [vp, ci, ci, C.POINTER(RslfStats)]
    L.rslf_multi_create.argtypes = [C.POINTER(ci), ci, C.POINTER(vp)]
    L.rslf_multi_destroy.argtypes = [vp]
    L.rslf_multi_device_count.argtypes = [vp]
    L.rslf_multi_set_chunk_rows.argtypes = [vp, ci]
    L.rslf_multi_peer_access.argtypes = [vp, ci, ci]
    L.rslf_debug_inject.argtypes = [C.c_char_p, ci]
    L.rslf_multi_depth1d_pile_f32.argtypes = [vp, C.POINTER(vp), C.c_size_t, ci, ci, ci, ci, cf, cf, cf, ci, ci, C.POINTER(RslfParams),
                                              vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(RslfStats), C.POINTER(cf)]
    L.rslf_multi_depth1d_pile_f32_dev.argtypes = [vp, C.POINTER(vp), C.c_size_t, ci, ci, ci, ci, cf, cf, cf, ci, ci, C.POINTER(RslfParams), ci,
                                                  vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(RslfStats), C.POINTER(cf)]
    L.rslf_multi_depth1d_pile_u8.argtypes = [vp, C.POINTER(vp), C.c_size_t, ci, ci, ci, ci, cf, cf, ci, ci, C.POINTER(RslfParams),
                                             vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(RslfStats)]
    L.rslf_multi_depth2d_run_f32.argtypes = [vp, C.POINTER(vp), C.c_size_t, ci, ci, ci, ci, cf, cf, cf, ci, C.POINTER(RslfParams),
                                             vp, vp, vp, vp, vp, vp, C.POINTER(RslfStats), C.POINTER(cf)]
    L.rslf_multi_depth1d_pile_u16.argtypes = L.rslf_multi_depth1d_pile_f32.argtypes
    L.rslf_multi_depth2d_run_u16.argtypes = L.rslf_multi_depth2d_run_f32.argtypes
    L.rslf_multi_depth2d_run_u8.argtypes = [vp, C.POINTER(vp), C.c_size_t, ci, ci, ci, ci, cf, cf, ci, C.POINTER(RslfParams),
                                            vp, vp, vp, vp, vp, vp, C.POINTER(RslfStats)]
    L.rslf_multi_fine_to_coarse_run_host.argtypes = [vp, C.POINTER(vp), ci, ci, ci, ci, ci, C.c_size_t, cf, cf, ci, cf, C.POINTER(RslfParams),
                                                     ci, ci, vp, vp, C.POINTER(ci), C.POINTER(RslfStats)]
    L.rslf_multi_fine_to_coarse_run_host_u16.argtypes = [vp, C.POINTER(vp), ci, ci, ci, ci, C.c_size_t, cf, cf, ci, cf,
                                                         C.POINTER(RslfParams), ci, ci, vp, vp, C.POINTER(ci), C.POINTER(RslfStats)]
    L.rslf_kernel_columns_pile.argtypes = [vp, vp, vp, vp, cf, cf, ci, ci, C.POINTER(RslfParams), vp, vp]
    L.rslf_depth2d_run_host.argtypes = [vp, vp, cf, cf, ci, C.POINTER(RslfParams), vp, vp, vp, vp, vp, C.POINTER(RslfStats)]
    L.rslf_fine_to_coarse_run_host.argtypes = [vp, C.POINTER(vp), ci, ci, ci, ci, ci, C.c_size_t, cf, cf, ci, cf, C.POINTER(RslfParams),
                                               ci, ci, vp, vp, C.POINTER(ci), C.POINTER(RslfStats)]
    L.rslf_fine_to_coarse_run_host_u16.argtypes = L.rslf_multi_fine_to_coarse_run_host_u16.argtypes
    L.rslf_f2c_pyramid_dims.argtypes = [ci, ci, ci, C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(ci)]
    L.rslf_fine_to_coarse_run_host_lc.argtypes = L.rslf_fine_to_coarse_run_host.argtypes + [ci, C.POINTER(RslfF2cLevelsOut)]
    L.rslf_fine_to_coarse_run_host_u16_lc.argtypes = L.rslf_fine_to_coarse_run_host_u16.argtypes + [ci, C.POINTER(RslfF2cLevelsOut)]
    L.rslf_f2c_run_host.argtypes = [vp, C.POINTER(vp), ci, ci, ci, ci, ci, C.c_size_t, cf, cf, ci, cf, C.POINTER(RslfParams), ci, ci, ci, ci, ci,
                                    C.POINTER(vp), C.POINTER(RslfStats)]
    L.rslf_f2c_run_destroy.argtypes = [vp]
    L.rslf_f2c_run_describe.argtypes = [vp, C.POINTER(RslfF2cRunDesc)]
    L.rslf_f2c_run_copy.argtypes = [vp, ci, ci, vp, ci, vp]
    L.rslf_f2c_run_volume.argtypes = [vp, ci, C.POINTER(vp)]
    L.rslf_f2c_run_render_depth_maps.argtypes = [vp, vp, ci, vp, vp]
    L.rslf_f2c_run_render_depth_maps_host.argtypes = L.rslf_f2c_run_render_depth_maps.argtypes
    L.rslf_f2c_run_render_depth_pyr.argtypes = [vp, vp, ci, ci, vp, C.POINTER(vp)]
    L.rslf_f2c_run_render_depth_pyr_host.argtypes = L.rslf_f2c_run_render_depth_pyr.argtypes
    L.rslf_f2c_run_render_epi_pyr.argtypes = L.rslf_f2c_run_render_depth_pyr.argtypes
    L.rslf_f2c_run_render_epi_pyr_host.argtypes = L.rslf_f2c_run_render_depth_pyr.argtypes
    L.rslf_f2c_level_dims.argtypes = [ci, ci, C.POINTER(ci), C.POINTER(ci)]
    L.rslf_downsample_epis_f32.argtypes = [vp, vp, ci, ci, ci, ci, vp]
    L.rslf_downsample_epis_u8.argtypes = [vp, vp, ci, ci, ci, ci, vp]
    L.rslf_downsample_epis_u16.argtypes = [vp, vp, ci, ci, ci, ci, vp]
    L.rslf_device_max_f32.argtypes = [vp, vp, C.c_size_t, C.POINTER(cf)]
    L.rslf_f2c_tighten_bounds.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, ci, ci]
    L.rslf_f2c_fuse.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(ci), C.POINTER(ci), ci, ci, vp, vp]
    L.rslf_render_fit.argtypes = [vp, vp, ci, ci, C.c_size_t, vp, ci, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rslf_render_planes.argtypes = [vp, vp, ci, C.c_size_t, ci, ci, C.c_size_t, C.c_double, C.c_double, ci, vp, vp, ci, vp, ci, ci, cf, vp]
    L.rslf_render_epi_lines.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp]
    L.rslf_render_epi_lines_host.argtypes = L.rslf_render_epi_lines.argtypes
    L.rslf_render_fit_many.argtypes = [vp, vp, ci, C.c_size_t, ci, ci, C.c_size_t, vp, ci, C.POINTER(C.c_double)]
    L.rslf_render_planes_each.argtypes = [vp, vp, ci, C.c_size_t, ci, ci, C.c_size_t, C.POINTER(C.c_double), ci, vp, vp, ci, vp, ci, ci, cf, vp]
    L.rslf_render_planes_host.argtypes = [vp, vp, ci, C.c_size_t, ci, ci, C.c_size_t, vp, ci, ci, ci, ci, vp, ci, vp, ci, ci, cf, vp,
                                          C.POINTER(C.c_double)]
    L.rslf_render_centre_index.argtypes = [ci, C.POINTER(ci)]
    L.rslf_render_scaled_row.argtypes = [ci, ci, ci, C.POINTER(ci)]
    L.rslf_edge_confidence_2d.argtypes = [vp, vp, C.POINTER(RslfParams), vp, vp]
    L.rslf_depth_epi_2d.argtypes = [vp, vp, vp, vp, cf, cf, ci, vp, vp, vp, vp, vp, C.POINTER(RslfParams), vp, C.POINTER(RslfStats)]
    L.rslf_depth2d_run.argtypes = [vp, vp, cf, cf, ci, C.POINTER(RslfParams), vp, vp, vp, vp, vp, vp, C.POINTER(RslfStats)]
    L.rslf_line_confidence_pile.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]
    L.rslf_sweep_line_confidence.argtypes = [vp, vp, ci, vp]
    L.rslf_depth_epi_2d_lc.argtypes = L.rslf_depth_epi_2d.argtypes + [ci, vp]
    L.rslf_depth2d_run_lc.argtypes = L.rslf_depth2d_run.argtypes + [ci, vp]
    L.rslf_depth2d_run_host_lc.argtypes = L.rslf_depth2d_run_host.argtypes + [ci, vp]
    L.rslf_sweep_subgrid.argtypes = [vp, vp, ci]
    L.rslf_depth_epi_2d_sub.argtypes = L.rslf_depth_epi_2d_lc.argtypes + [ci]
    L.rslf_depth2d_run_sub.argtypes = L.rslf_depth2d_run_lc.argtypes + [ci]
    L.rslf_depth2d_run_host_sub.argtypes = L.rslf_depth2d_run_host_lc.argtypes + [ci]
    L.rslf_fine_to_coarse_run_host_sub.argtypes = L.rslf_fine_to_coarse_run_host_lc.argtypes + [ci]   # (elem where is_u8 is: an int too)
    L.rslf_f2c_run_host_sub.argtypes = L.rslf_f2c_run_host.argtypes + [ci]
    L.rslf_f2c_run_subgrid.argtypes = [vp]
    L.rslf_sweep_peaks.argtypes = [vp, vp, vp]
    L.rslf_depth_epi_2d_pk.argtypes = L.rslf_depth_epi_2d_sub.argtypes + [vp]
    L.rslf_depth2d_run_pk.argtypes = L.rslf_depth2d_run_sub.argtypes + [vp]
    L.rslf_depth2d_run_host_pk.argtypes = L.rslf_depth2d_run_host_sub.argtypes + [vp]
    L.rslf_f2c_run_host_pk.argtypes = L.rslf_f2c_run_host_sub.argtypes + [ci, cf]
    L.rslf_sweep_propagation_ratio.argtypes = [vp, vp, cf]
    L.rslf_sweep_withheld.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    L.rslf_depth_epi_2d_pr.argtypes = L.rslf_depth_epi_2d_pk.argtypes + [cf]
    L.rslf_depth2d_run_pr.argtypes = L.rslf_depth2d_run_pk.argtypes + [cf]
    L.rslf_depth2d_run_host_pr.argtypes = L.rslf_depth2d_run_host_pk.argtypes + [cf]
    L.rslf_f2c_run_host_pr.argtypes = L.rslf_f2c_run_host_pk.argtypes + [cf]
    L.rslf_f2c_run_propagation_ratio.argtypes = [vp]
    L.rslf_f2c_run_propagation_ratio.restype = cf
    L.rslf_f2c_run_withheld.argtypes = [vp, ci, C.POINTER(C.c_ulonglong)]
    L.rslf_view_consistency.argtypes = [vp, vp, vp, ci, ci, ci, cf, cf, ci, ci, C.POINTER(RslfViewCounts), vp, vp]
    L.rslf_view_consistency_host.argtypes = L.rslf_view_consistency.argtypes
    L.rslf_f2c_run_consistency.argtypes = [vp, vp, ci, ci, cf, ci, ci, C.POINTER(RslfViewCounts), vp, vp]
    L.rslf_f2c_run_consistency_host.argtypes = L.rslf_f2c_run_consistency.argtypes
    L.rslf_f2c_run_host_cs.argtypes = L.rslf_f2c_run_host_pr.argtypes + [cf, ci, ci]
    L.rslf_f2c_run_host_dv.argtypes = L.rslf_f2c_run_host_cs.argtypes + [cf]
    L.rslf_fine_to_coarse_run_host_dv.argtypes = L.rslf_fine_to_coarse_run_host_sub.argtypes + [cf]
    L.rslf_f2c_run_host_dl.argtypes = L.rslf_f2c_run_host_dv.argtypes + [ci, ci]
    L.rslf_fine_to_coarse_run_host_dl.argtypes = L.rslf_fine_to_coarse_run_host_dv.argtypes + [ci, ci]
    L.rslf_f2c_run_level_dilation.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
    L.rslf_f2c_run_host_eq.argtypes = L.rslf_f2c_run_host_dl.argtypes + [ci, ci, ci, cf]
    L.rslf_fine_to_coarse_run_host_eq.argtypes = L.rslf_fine_to_coarse_run_host_dl.argtypes + [ci, ci, ci, cf]
    L.rslf_f2c_run_equalize.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), vp]
    L.rslf_f2c_run_view_gains_channels.argtypes = [vp]
    L.rslf_apply_view_gains_dense.argtypes = [vp, vp, ci, ci, ci, ci, ci, cf, vp, vp]
    L.rslf_volume_view_stats.argtypes = [vp, vp, vp, C.POINTER(cf)]
    L.rslf_view_stats_dense.argtypes = [vp, vp, ci, ci, ci, ci, ci, cf, vp]
    L.rslf_equalize_coefficients.argtypes = [vp, ci, ci, cf, ci, ci, ci, cf, vp]
    L.rslf_volume_equalize_views.argtypes = [vp, vp, ci, ci, ci, cf, C.POINTER(vp), vp]
    L.rslf_volume_apply_view_gains.argtypes = [vp, vp, vp, C.POINTER(vp)]
    L.rslf_equalize_views_dense.argtypes = [vp, vp, ci, ci, ci, ci, ci, cf, ci, ci, ci, cf, vp]
    L.rslf_volume_derivative_channels.argtypes = [vp, vp, cf, C.POINTER(vp)]
    L.rslf_derivative_channels_dense.argtypes = [vp, vp, ci, ci, ci, ci, cf, cf, vp]
    L.rslf_f2c_run_consistency_gate.argtypes = [vp, C.POINTER(cf), C.POINTER(ci), C.POINTER(ci)]
    L.rslf_f2c_run_inconsistent.argtypes = [vp, ci, C.POINTER(C.c_ulonglong)]
    L.rslf_f2c_consistency_mask.argtypes = [vp, vp, vp, ci, ci, ci, cf, cf, ci, ci, vp, vp, vp, vp]
    L.rslf_view_warp.argtypes = [vp, vp, vp, ci, ci, ci, cf, vp, C.POINTER(cf), C.POINTER(ci), ci, ci, ci, C.POINTER(RslfViewWarpOut)]
    L.rslf_view_warp_host.argtypes = L.rslf_view_warp.argtypes
    L.rslf_f2c_run_view_warp.argtypes = [vp, vp, ci, ci, C.POINTER(cf), C.POINTER(ci), ci, ci, ci, C.POINTER(RslfViewWarpOut)]
    L.rslf_f2c_run_view_warp_host.argtypes = L.rslf_f2c_run_view_warp.argtypes
    L.rslf_novel_view.argtypes = [vp, vp, vp, ci, ci, ci, cf, vp, C.POINTER(cf), C.POINTER(ci), ci, C.POINTER(RslfNovelViewParams),
                                  C.POINTER(RslfNovelViewOut)]
    L.rslf_novel_view_host.argtypes = L.rslf_novel_view.argtypes
    L.rslf_f2c_run_novel_view.argtypes = [vp, vp, ci, ci, C.POINTER(cf), C.POINTER(ci), ci, C.POINTER(RslfNovelViewParams),
                                          C.POINTER(RslfNovelViewOut)]
    L.rslf_f2c_run_novel_view_host.argtypes = L.rslf_f2c_run_novel_view.argtypes
    L.rslf_dilated_width.argtypes = [ci, ci, C.POINTER(ci)]
    L.rslf_volume_dilate_u.argtypes = [vp, vp, ci, ci, C.POINTER(vp)]
    L.rslf_planes_undilate_u.argtypes = [vp, vp, ci, C.c_size_t, ci, ci, vp]
    L.rslf_planes_undilate_u_host.argtypes = [vp, C.c_size_t, ci, C.c_size_t, ci, ci, vp, C.c_size_t]
    L.rslf_planes_dilate_ranges_u.argtypes = [vp, vp, vp, C.c_size_t, ci, ci, vp, vp]
    L.rslf_planes_dilate_ranges_u_host.argtypes = [vp, vp, C.c_size_t, C.c_size_t, ci, ci, vp, vp, C.c_size_t]
    L.rslf_planes_undilate_many_u.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(ci), ci, C.c_size_t, ci, ci]
    L.rslf_f2c_run_peaks.argtypes = [vp]
    L.rslf_f2c_run_uniqueness.argtypes = [vp]
    L.rslf_f2c_run_uniqueness.restype = cf
    L.rslf_f2c_unique_mask.argtypes = [vp, vp, C.POINTER(RslfPeaks), cf, C.c_size_t]
    L.rslf_f2c_fuse_peaks.argtypes = [vp, C.POINTER(vp), C.POINTER(RslfPeaks), C.POINTER(ci), C.POINTER(ci), ci, ci, C.POINTER(RslfPeaks), vp]
    for name in SYMBOLS:
        f = getattr(L, name)   # AttributeError here = the library does not export the ABI
        if f.restype is C.c_int and name not in ("rslf_abi_version", "rslf_device_count"):
            pass
    if L.rslf_abi_version() != ABI_VERSION:
        raise RuntimeError("librslf_hip.so has ABI %d, binding expects %d" % (L.rslf_abi_version(), ABI_VERSION))
    _LIB = L
    return L


def check(status: int, where: str) -> None:
    if status != 0:
        raise RslfError(status, where)


def default_params() -> RslfParams:
    p = RslfParams()
    lib().rslf_default_params(C.byref(p))
    return p
