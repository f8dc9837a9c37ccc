/*
 * rslf_hip.h -- C-ABI of the MI355X-native EPI depth scan.
 *
 * This is the drop-in boundary for ONE path of RSLightFields
 * (14chanwa/remotesensingProject): everything below
 * rslf::Depth1DComputer_pile<T>::run() -- the scanline-parallel edge
 * confidence, the per-pixel x per-hypothesis EPI-slope scan with its mean
 * shift, and the selective median -- runs as hand-written HIP kernels for
 * gfx950.  The reference has no FFI of its own (it is one C++11/OpenCV/OpenMP
 * library); the seam is the template free-function signatures cited per entry
 * point below (paths relative to /root/reference/RSLightFields/).  The C++11
 * host class that keeps the reference's constructor/run() shape is
 * include/rslf_hip.hpp; the binding a maintainer would add on the reference
 * side is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C, no C++/torch/OpenCV types; every function returns an rslf_status
 *    (0 = ok, <0 = error) and never throws across the boundary: every entry
 *    point is a function-try-block (std::bad_alloc -> RSLF_ERR_ALLOC, anything
 *    else -> RSLF_ERR_INTERNAL), and worker threads are joined on every path.
 *    (The reference returns void and has no error convention: SURVEY.md 8b.)
 *  - pointers named d_* are DEVICE pointers, h_* are HOST pointers; all
 *    buffers are caller-owned; planes are dense row-major [V][U].
 *  - work is enqueued on the context's stream (rslf_ctx_set_stream, a
 *    hipStream_t passed as void*); *_host entry points synchronise before
 *    returning, device entry points do not.
 *  - a context is not re-entrant; use one per host thread / stream.
 *  - there is NO CPU fallback behind this ABI.
 */
#ifndef RSLF_HIP_H
#define RSLF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSLF_ABI_VERSION 6

typedef enum rslf_status {
    RSLF_OK = 0,
    RSLF_ERR_INVALID_ARG = -1,   /* null pointer, bad dimension, dim_d < 2, ... */
    RSLF_ERR_UNSUPPORTED = -2,   /* channel count other than 1 or 3, filter sizes the kernels do not cover */
    RSLF_ERR_HIP = -3,           /* a HIP runtime call failed; see rslf_last_error() */
    RSLF_ERR_NO_DEVICE = -4,     /* no gfx950 device visible */
    RSLF_ERR_ALLOC = -5,         /* device or host memory could not be had (hipMalloc, std::bad_alloc) */
    RSLF_ERR_INTERNAL = -6       /* a C++ exception was stopped at the boundary; its text is in rslf_last_error() */
} rslf_status;

/* Mirrors rslf::Depth1DParameters<T> -- include/rslf_depth_computation_core.hpp:66-142
 * (defaults :16-31, :74-99).  Same member meaning, par_ prefix dropped.  The two
 * polymorphic plug-ins (:108-109) become plain members: `interpolation` selects
 * between the reference's two interpolation classes (include/rslf_interpolation.hpp),
 * and the kernel is BandwidthKernel(h) (src/rslf_kernels.cpp:16-54), h = kernel_bandwidth. */
typedef struct rslf_params {
    float edge_score_threshold;         /* 0.02 */
    float line_score_threshold;         /* 0.02  (the gate of RSLF_LINE_CONF_GATE sweeps) */
    float disp_score_threshold;         /* 0.01  (only with use_disp_confidence_score) */
    float raw_score_threshold;          /* 0 */
    float mean_shift_max_iter;          /* 10; a float in the reference (:115) */
    int   edge_confidence_filter_size;  /* 9 */
    int   edge_confidence_opening_type; /* cv::MORPH_RECT 0 / MORPH_CROSS 1 / MORPH_ELLIPSE 2 (default) */
    int   edge_confidence_opening_size; /* 1 = no morphological opening (default); k in 2..31: cv::morphologyEx(MORPH_OPEN)
                                           with getStructuringElement(type, Size(k, k)) on the edge mask (core.hpp:759-768) */
    int   median_filter_size;           /* 5; any size >= 0: window half-width (size - 1) / 2, core.hpp:686 */
    float median_filter_epsilon;        /* 0.1 */
    float propagation_epsilon;          /* 0.1 (unused by this path) */
    float slope_factor;                 /* 1.0 */
    int   cut_shadows;                  /* 1 */
    float shadow_level;                 /* 0.05 * 1.73205080757 */
    float kernel_bandwidth;             /* 0.2 (_BANDWIDTH_KERNEL_PARAMETER, :26) */
    int   interpolation;                /* par_interpolation_class (:76-77, :108): RSLF_INTERP_*, default LINEAR */
    int   use_disp_confidence_score;    /* the reference's commented-out build switch _USE_DISP_CONFIDENCE_SCORE (:35): the 2-D
                                           sweep's propagation is gated by C_d > disp_score_threshold (:1097-1098) instead of the
                                           edge mask (:1102).  0 = the default build */
} rslf_params;

/* par_interpolation_class.
 * LINEAR            Interpolation1DLinear (include/rslf_interpolation.hpp:155-193), the reference default.
 * NEAREST           Interpolation1DNearestNeighbour as its scalar interpolate() states it (:80-92):
 *                   index (int)std::round(x), NaN outside [0, U-1].
 * NEAREST_AS_BUILT  what its interpolate_mat() -- the method the scan calls (core.hpp:561) -- executes:
 *                   the float index matrix is read through `indices.ptr<int>` (:118), so the "index" is
 *                   the BIT PATTERN of x, in range only for x = +0.  Kept so that a caller who selects
 *                   the reference's commented-out line (core.hpp:77) gets the reference's result bit for bit.
 * The two nearest modes run on the generic scan kernel only. */
#define RSLF_INTERP_LINEAR            0
#define RSLF_INTERP_NEAREST           1
#define RSLF_INTERP_NEAREST_AS_BUILT  2

typedef struct rslf_ctx rslf_ctx;       /* device, stream, scratch */
typedef struct rslf_volume rslf_volume; /* light-field slab resident in HBM */

typedef struct rslf_volume_desc {
    int V, S, U, C;       /* scanlines, views, columns, channels */
    int pitch;            /* floats per (v,s,c) row, multiple of 64, > U (zero padded) */
    void* d_base;         /* device address of element (v=0,s=0,c=0,u=0) */
    size_t bytes;         /* allocation size */
    float min_value;      /* over the normalised volume */
    float max_value;
} rslf_volume_desc;

/* Per-call statistics (nullable wherever taken). */
typedef struct rslf_stats {
    int64_t pixels_scanned;   /* pixels whose scan mask was set on entry (core.hpp:515-527) */
    int64_t units;            /* pixels_scanned * dim_d  = (pixel, hypothesis) pairs */
    int     scan_kernel;      /* which K2 variant ran: see RSLF_SCAN_* */
    int     s_pad;            /* register slots per lane of the register variant, else 0 */
} rslf_stats;

#define RSLF_SCAN_GENERIC   0  /* any S, C in {1,3}, any sign: re-gathers every mean-shift pass */
#define RSLF_SCAN_STREAM    2  /* volume >= 0, any S: a resident prefix of the samples (registers + LDS), the rest re-gathered every pass */
#define RSLF_SCAN_REG       1  /* volume >= 0 and C=1, S<=192 or C=3, S<=48: every sample held in registers */
#define RSLF_SCAN_CHIP      3  /* volume >= 0, C=3, S in [123, 220], dense launch with one hypothesis grid: one wave per SIMD, all but
                                  three samples of a unit on chip (VGPRs + AGPRs + LDS, a ladder of instantiations 8 views apart;
                                  201 views = BASELINE.json's c5 is the top rung), packed-fp32 passes */
#define RSLF_SCAN_REG_PX    4  /* RSLF_SCAN_REG's shapes on a packed (sparse) launch: a wave owns one pixel, its lanes the hypotheses */
#define RSLF_SCAN_STREAM_PX 5  /* RSLF_SCAN_STREAM's shapes on a packed (sparse) launch, the same way */

int         rslf_abi_version(void);
const char* rslf_status_string(int status);
const char* rslf_last_error(void);       /* thread-local text of the last failure */
int         rslf_device_count(void);
/* rslf::Depth1DParameters<T>::Depth1DParameters() -- core.hpp:74-99 */
void        rslf_default_params(rslf_params* p);

/* ---- context ---------------------------------------------------------- */
int rslf_ctx_create(int device, rslf_ctx** out);
int rslf_ctx_destroy(rslf_ctx* ctx);
int rslf_ctx_set_stream(rslf_ctx* ctx, void* hip_stream);   /* NULL = default stream */
int rslf_ctx_synchronize(rslf_ctx* ctx);
/* Test and tuning hooks of ONE context (nothing process-global, no environment variable is read):
 *   "force_scan"     0 automatic | 1 generic scan kernel | 2 streaming scan kernel (never the on-chip one)
 *   "force_groups"   0 automatic | 1..64 hypothesis groups per tile
 *   "force_packed"   -1 automatic | 0 row tiles | 1 one packed pixel list
 *   "px"             -1 automatic | 0 never | 1 whenever it can run: packed launches of a register or streaming kernel put a pixel's
 *                    HYPOTHESES in the lanes of a wave (k2_scan_reg_px, k2_scan_stream_px) instead of 64 pixels
 *   "row_split"      1 (default) packed launches of stream-class volumes scan the rows that hold >= 64 pixels as row tiles of
 *                    the packed list and leave the pixel-per-wave launch the rest | 0 the pixel-per-wave launch takes all
 *   "tap_table"      1 (default) the register row kernels that have one (k2_scan_reg<104,1>) take the lerp taps and weights that
 *                    are the same in every lane of a tile from a per-hypothesis table | 0 every lane computes its own
 *   "scalar_taps"    1 (default) with "tap_table" on, hypotheses whose lerp taps and weights are the same for every pixel of the row
 *                    take them as scalars from a table made once per hypothesis grid and kept by the context | 0 off
 *   "claim_skip"     1 (default) the 2-D sweep's claims skip views with nothing left to paint within reach | 0 off
 *   "subgrid_list"   1 (default) a 2-D sweep in the sub-grid mode (rslf_sweep_subgrid) refines a visit whose scan took the packed
 *                    list over that list | 0 every visit refines over the whole plane (k9_subgrid_refine), the same bits
 *   "peaks_list"     1 (default) a 2-D sweep in the peaks mode (rslf_sweep_peaks) takes the peaks of a visit whose scan took the
 *                    packed list over that list (k10_peaks_list) | 0 every visit takes the dense form, the same bits
 *   "consistency_order"  0 (default) rslf_view_consistency's workgroups in scanline order, the scanlines dealt to the XCDs in
 *                    turn | 1 scanline order as dispatched | 2 the planes' own order (profiles/r19_consistency.md)
 *   "stream_share"   63-pixel tiles sharing taps between lanes in the streaming kernel: 1 (default) where the samples gathered
 *                    again on every pass are at least a quarter of the views | 0 never | 2 always
 *   "stream_groups"  0 automatic | hypothesis groups per tile of the streaming kernel's dense launches
 *   "stream_lds_kib" dynamic LDS of one streaming workgroup, KiB (default 80)
 *   "time_all"       0 (default) | 1: every scan launch is bracketed by its own pair of HIP events, summed and reset by
 *                    rslf_scan_time_total_ms (the K2 time of a whole sweep or pyramid; each event costs ~5.6 us in the queue)
 *   "staging_kib"    0 (default) the host uploads of a volume walk it in passes through 256 MiB of device staging | 1..262144:
 *                    that budget in KiB (a pass holds at least one scanline), so that a small volume takes several passes
 * Results do not depend on these (the parity tests drive every combination; "claim_skip" on / off is compared plane by
 * plane in tests/test_gpu_sweep2d.py); speed does.  One qualification: the disparity confidence C_d = C_e * |max - mean of
 * the scores| takes the mean through a double sum whose ORDER differs between launch shapes (per wave in the row kernels,
 * a butterfly over lanes in k2_scan_reg_px / k2_scan_stream_px); sums of <= 4096 floats in [0, 1] are exact in a double
 * unless a score is below 2^-21, so C_d of two launch shapes is equal to within 1e-5 (the tolerance the reference's float
 * output is held to), not guaranteed bitwise.  Every other plane -- masks, arg-max indices, disparities, scores, r-bar,
 * C_e -- is bit-identical whatever the hooks say. */
int rslf_ctx_set_debug(rslf_ctx* ctx, const char* key, int value);
/* Fault injection for the tests of the error paths (process-wide, off unless armed): the next `count` visits of `site`
 * fail as if the runtime had -- "worker": a device worker of rslf_multi_* throws std::runtime_error; "thread_create":
 * std::thread cannot be started (the work then runs on the calling thread); "alloc": std::bad_alloc in a worker; "sweep":
 * rslf_multi_depth2d_run_* throws std::runtime_error once every device's sweep is open, before the first visit is queued,
 * and so does a level of the one-context fine-to-coarse loop before its sweep is queued.
 * The entry point reports a status; nothing is left running, nothing leaks.  count = 0 disarms. */
int rslf_debug_inject(const char* site, int count);

/* ---- volume: replaces Depth1DComputer_pile's constructor --------------- */
/* include/rslf_depth_computation.hpp:425-477: the constructor copies the
 * caller's Vec<Mat> of V EPIs (each S x U, C channels interleaved) into float
 * Mats scaled to [0,1].  Here the copy lands in one HBM slab laid out
 * [V][S][pitch][C]: one zero-padded row of `pitch` pixels per (EPI, view), channels
 * interleaved like the reference's Mat rows, so the two lerp taps of a sample, all
 * channels, are 2*C consecutive floats. */
int rslf_volume_create(rslf_ctx* ctx, int V, int S, int U, int C, rslf_volume** out);
int rslf_volume_destroy(rslf_volume* vol);   /* waits for the device; contexts and volumes may be destroyed in either order */
int rslf_volume_describe(const rslf_volume* vol, rslf_volume_desc* out);

/* ---- dilation along u (K16; not in the reference's code: the fourth lead of its report) ---- */
/* Small slopes put most of a line's samples at sub-pixel offsets, where the scan's 2-tap lerp blurs each by an amount that
 * depends on the offset.  The remedy is to resample the volume once along u by an integer factor with a good kernel and to
 * run every path unchanged with slope_factor * factor (params.slope_factor is the caller's to set).
 *   U' = factor * (U - 1) + 1; output column i * factor + p lies at source coordinate i + p / factor.
 *   Phase 0 copies source column i bit for bit (factor 1 copies the volume).  Every other phase is a sum of T = 2 R taps,
 *   acc = w[0] * x[i - R + 1], then acc += w[m] * x[i - R + 1 + m] for ascending m (binary32 multiply, then add), indices
 *   clamped to [0, U - 1], and out = min(max(acc, min_value), max_value) of the source: the new volume has the source's
 *   min_value and max_value exactly, and a non-negative volume stays one (RSLF_SCAN_* above).  The weights are the kind's
 *   kernel h(p / factor - (m - R + 1)) in double, divided by their double sum, rounded to float.  Channels are independent. */
#define RSLF_DILATE_LINEAR    0   /* R = 1: the lerp (what the scan does by itself: changes nothing) */
#define RSLF_DILATE_CUBIC     1   /* R = 2: Keys' cubic convolution, a = -0.5 */
#define RSLF_DILATE_LANCZOS3  2   /* R = 3: sinc(x) * sinc(x / 3) */
/* *U_out = factor * (U - 1) + 1.  RSLF_ERR_INVALID_ARG: U < 1, factor outside 1..8, NULL; RSLF_ERR_UNSUPPORTED: U' and its pad
 * do not fit an int (rslf_volume_dilate_u also applies rslf_volume_create's limits to the new volume). */
int rslf_dilated_width(int U, int factor, int* U_out);
/* A new volume [V][S][U'][C] from a filled one of the same context's device; enqueued on the context's stream, not awaited.
 * The new volume is the caller's (rslf_volume_destroy).  A failed call leaves *out NULL and frees what it allocated --
 * except where *out IS src on entry (the call would overwrite the source's handle): refused, *out untouched.
 * RSLF_ERR_INVALID_ARG: NULL, factor outside 1..8, an unknown kind, a source never filled, a source of another device. */
int rslf_volume_dilate_u(rslf_ctx* ctx, const rslf_volume* src, int factor, int kind, rslf_volume** out);
/* d_out[r][u] = d_in[r][u * factor]: planes [rows][U_dilated] of the dilated frame on the source grid, [rows][U], dense.
 * elem_bytes 1 (masks) or 4 (float, int32).  Enqueued, not awaited.  RSLF_ERR_INVALID_ARG: NULL, d_out == d_in, elem_bytes
 * other than 1 or 4, factor outside 1..8, U_dilated not factor * (U - 1) + 1 for an integer U >= 1. */
int rslf_planes_undilate_u(rslf_ctx* ctx, const void* d_in, int elem_bytes, size_t rows, int U_dilated, int factor, void* d_out);
/* The same on host pointers, rows `*_row_stride_bytes` apart (0: dense).  A strided copy on the calling thread: no context,
 * no device.  Also refuses a stride shorter than its row. */
int rslf_planes_undilate_u_host(const void* h_in, size_t in_row_stride_bytes, int elem_bytes, size_t rows, int U_dilated, int factor,
                                void* h_out, size_t out_row_stride_bytes);
/* K18, what a fine-to-coarse level needs around a sweep in the dilated frame (the level dilation, below).
 * The per-pixel ranges dmin, dmax [rows][U] in the dilated frame, [rows][U'], dense: column i * factor + p takes
 * dmin[i] and dmax[i] bit for bit when p == 0, else fminf(dmin[i], dmin[i + 1]) and fmaxf(dmax[i], dmax[i + 1]) -- the
 * union of the two neighbours' ranges, so no hypothesis either allowed is lost; of two equal values (-0.0f, +0.0f) the left
 * one's bits, and a NaN loses to a number (csrc/k18_ranges_rule.hpp).  Both planes in one launch, enqueued on the context's
 * stream, not awaited.  RSLF_ERR_INVALID_ARG: NULL, an output plane that is an input plane or the other output, U < 1, factor
 * outside 1..8; RSLF_ERR_UNSUPPORTED: U' does not fit a row. */
int rslf_planes_dilate_ranges_u(rslf_ctx* ctx, const float* d_dmin, const float* d_dmax, size_t rows, int U, int factor,
                                float* d_dmin_out, float* d_dmax_out);
/* The same on host pointers, rows `*_row_stride_bytes` apart (0: dense; a multiple of 4): a loop on the calling thread, no
 * context, no device.  Also refuses a stride shorter than its row. */
int rslf_planes_dilate_ranges_u_host(const float* h_dmin, const float* h_dmax, size_t in_row_stride_bytes, size_t rows, int U,
                                     int factor, float* h_dmin_out, float* h_dmax_out, size_t out_row_stride_bytes);
/* rslf_planes_undilate_u for n_planes planes of the same rows and widths in ONE launch: d_out[k][r][u] =
 * d_in[k][r][u * factor], plane k of elem_bytes[k] (1 or 4) bytes per element; at most 8 planes of 4-byte and 2 of 1-byte
 * elements.  d_in, d_out and elem_bytes are HOST arrays, read before the return.  Enqueued, not awaited.  Refusals:
 * rslf_planes_undilate_u's per plane, more planes than that, an output plane that is any input or another output. */
int rslf_planes_undilate_many_u(rslf_ctx* ctx, const void* const* d_in, void* const* d_out, const int* elem_bytes, int n_planes,
                                size_t rows, int U_dilated, int factor);

/* ---- derivative channels (K17; not in the reference's code: the second lead of its report) ---- */
/* Every level down the pyramid, the Gaussian and the halving erase fine texture, and the edge confidence of the coarse
 * levels -- the ones meant to decide what the fine levels could not -- falls under its threshold.  The absolute
 * derivatives of the image, taken once at the finest level and carried down by the same downsample, survive where the
 * intensity has gone flat (averaging an absolute value is not linear).  A one-channel field x[v][s][u] becomes three
 * channels per pixel, (x, fu, fv):
 *   h  = 0.5f * weight                                    (float, once)
 *   fu = cap(fabsf(x[v][s][min(u+1, U-1)] - x[v][s][max(u-1, 0)]) * h, hi)
 *   fv = cap(fabsf(x[min(v+1, V-1)][s][u] - x[max(v-1, 0)][s][u]) * h, hi)
 * one binary32 subtraction, fabsf, one binary32 multiplication; cap(f, hi) = f > hi ? hi : f.  Channel 0 is the source's
 * bits; U == 1 gives fu = 0, V == 1 gives fv = 0; the neighbour along v is another EPI, the image's second spatial axis.
 * Float elements: hi = max(m, 0), m the source's maximum, so the maximum -- and a level's epi_scale_factor -- stays the
 * intensity's.  Integer elements (RSLF_ELEM_U8 / _U16: the pyramid's raw levels, integer values held as floats): the
 * product goes through rintf, ties to even, as cv::saturate_cast rounds, and hi is 255 or 65535.
 *
 * rslf_volume_derivative_channels: a new volume [V][S][U][3] from a filled one-channel volume of the same context's device
 * (hi from its max_value); the kernel is enqueued on the context's stream, and the call then waits for the two floats of the
 * new slab's range, as the uploads do: min_value and max_value are the new slab's own (the maximum is the source's by the
 * cap).  The new volume is the caller's (rslf_volume_destroy).  A failed call leaves *out NULL and frees what it allocated --
 * except where *out IS src on entry (the call would overwrite the source's handle): refused, *out untouched.
 * RSLF_ERR_INVALID_ARG: NULL, a weight that is not finite or is <= 0, a source never filled, a source of another device;
 * RSLF_ERR_UNSUPPORTED: a source of three channels. */
int rslf_volume_derivative_channels(rslf_ctx* ctx, const rslf_volume* src, float weight, rslf_volume** out);
/* The same on device pointers: a dense level d_in_vsu [V][S][U] of element type `elem` (RSLF_ELEM_*; always floats in
 * memory) becomes d_out_vsu3 [V][S][U][3].  hi: the cap of float elements, not a NaN and >= 0 (the caller's max(m, 0));
 * ignored for integer elements, whose cap is their type's.  Enqueued, not awaited.  RSLF_ERR_INVALID_ARG: NULL,
 * d_out_vsu3 == d_in_vsu, an unknown elem, a bad weight or hi, a dimension < 1; RSLF_ERR_UNSUPPORTED: 3 * U or V * S beyond an int. */
int rslf_derivative_channels_dense(rslf_ctx* ctx, const float* d_in_vsu, int elem, int V, int S, int U, float weight, float hi,
                                   float* d_out_vsu3);

/* ---- per-view equalisation (K19; not in the reference's code: the remedy its report names for global changes of
 * illumination between frames, "some preprocessing equalization") ---- */
/* A sample votes for a line only while its radiance lies within kernel_bandwidth of the running mean, so a view whose gain
 * has drifted stops voting.  The remedy is one (a, b) per view s and channel c, y = a x + b, from one statistic over all
 * (v, u) of the view.  The rule (csrc/k19_equalize_rule.hpp) is stated so that any correct implementation gives the same bits:
 *   Statistics, on integers: hi > 0 is the field's cap (a volume: its max_value; integer elements: 255 or 65535; float
 *   elements of a dense level: the caller's, e.g. rslf_device_max_f32), k = 65535.0f / hi one binary32 division, and
 *     q(x) = (uint32) min(rintf(fminf(fmaxf(x, 0.f), hi) * k), 65535.f);      a NaN sample is not counted;
 *   per (s, c) over all v and u < U: n = #counted, s1 = sum q, s2 = sum q^2, three uint64, exact while V * U <= 2^31 - 1.
 *   Coefficients, on the host in double: m = s1 / n / 65535 * hi, var = max(s2 / n / 65535^2 * hi^2 - m^2, 0), sd = sqrt(var);
 *   joint (C == 3 only) adds the three channels' n, s1, s2 first and writes the one pair to all three (hue is kept); the
 *   target (mt, sdt) is view ref_view's (m, sd) or, ref_view == -1, the arithmetic mean of m and of sd over the views with
 *   n > 0.  RSLF_EQUALIZE_GAIN: a = m > 0 ? mt / m : 1, b = 0.  RSLF_EQUALIZE_AFFINE: a = sd > 0 ? sdt / sd : 1, b = mt - a m.
 *   a is clamped to [1 / max_gain, max_gain] and b computed after the clamp; a view with n == 0, the reference view itself,
 *   and every view of a field whose target has no sample get exactly (1, 0); a and b are rounded to float once, at the end.
 *   Apply: y = x * a + b (one binary32 multiplication, one addition), integer elements then rintf (ties to even), then
 *   y < 0 ? 0 : (y > hi ? hi : y); a NaN stays that NaN; a pair (1, 0) copies the source's bits. */
#define RSLF_EQUALIZE_GAIN    1
#define RSLF_EQUALIZE_AFFINE  2
/* The statistics of a filled volume of the context's device into h_stats [S][C][3] (n, s1, s2), hi = the volume's max_value
 * (also left in *hi_used, nullable).  Awaited.  RSLF_ERR_INVALID_ARG: NULL, a volume never filled or of another device;
 * RSLF_ERR_UNSUPPORTED: V * U beyond 2^31 - 1, a volume whose min_value < 0 (or that holds a NaN) or whose max_value is not
 * finite and > 0. */
int rslf_volume_view_stats(rslf_ctx* ctx, const rslf_volume* vol, uint64_t* h_stats, float* hi_used);
/* The same of a dense level d_in_vsuc [V][S][U][C] of element type `elem` (RSLF_ELEM_*; always floats in memory) into the
 * DEVICE buffer d_stats [S][C][3] (8-byte aligned), which the call zeroes first.  hi: the cap of float elements, finite and
 * > 0; ignored for integer elements.  Enqueued on the context's stream, not awaited.  RSLF_ERR_INVALID_ARG: NULL, an unknown
 * elem, a bad hi, a dimension < 1, C other than 1 or 3; RSLF_ERR_UNSUPPORTED: V * U beyond 2^31 - 1. */
int rslf_view_stats_dense(rslf_ctx* ctx, const float* d_in_vsuc, int elem, int V, int S, int U, int C, float hi, uint64_t* d_stats);
/* h_stats [S][C][3] -> h_a_b [S][C][2] by the rule above.  No context and no device: it works on a machine without a GPU.
 * RSLF_ERR_INVALID_ARG: NULL, S < 1, C other than 1 or 3, a hi that is not finite and > 0, an unknown mode, ref_view outside
 * [-1, S), a max_gain that is not finite or < 1, joint with C == 1. */
int rslf_equalize_coefficients(const uint64_t* h_stats, int S, int C, float hi, int mode, int ref_view, int joint, float max_gain,
                               float* h_a_b);
/* Statistics, coefficients, apply: a new volume [V][S][U][C] from a filled one of the same context's device.  The call waits
 * for the S * C * 3 integers between the two kernels and then for the two floats of the new slab's range, as the uploads do;
 * the pad is written as zeros.  h_a_b [S][C][2] receives the coefficients (nullable).  *out has rslf_volume_dilate_u's
 * contract: the caller's on success, NULL after a failed call, and a call whose *out IS src on entry is refused, *out
 * untouched.  RSLF_ERR_INVALID_ARG: NULL, an unknown mode, ref_view outside [-1, S), a max_gain that is not finite or < 1,
 * joint with C == 1, a source never filled or of another device; RSLF_ERR_UNSUPPORTED as rslf_volume_view_stats. */
int rslf_volume_equalize_views(rslf_ctx* ctx, const rslf_volume* src, int mode, int ref_view, int joint, float max_gain,
                               rslf_volume** out, float* h_a_b);
/* The apply pass alone, with the caller's coefficients h_a_b [S][C][2] (from a masked statistic of their own, say), all
 * finite; hi is the source's max_value.  Contract and refusals as above. */
int rslf_volume_apply_view_gains(rslf_ctx* ctx, const rslf_volume* src, const float* h_a_b, rslf_volume** out);
/* The three steps on a dense level d_inout_vsuc [V][S][U][C], in place, awaited.  hi as rslf_view_stats_dense; h_a_b nullable.
 * Refusals: rslf_view_stats_dense's and rslf_volume_equalize_views's of the options. */
int rslf_equalize_views_dense(rslf_ctx* ctx, float* d_inout_vsuc, int elem, int V, int S, int U, int C, float hi, int mode,
                              int ref_view, int joint, float max_gain, float* h_a_b);
/* The apply pass alone on a dense level, with the caller's coefficients h_a_b [S][C][2] (a HOST array, all finite, read
 * before the return): d_out_vsuc = a x + b of d_in_vsuc; d_out_vsuc may be d_in_vsuc.  hi as rslf_view_stats_dense.  Enqueued
 * on the context's stream, not awaited.  RSLF_ERR_INVALID_ARG: NULL, an unknown elem, a bad hi, a coefficient that is not
 * finite, a dimension < 1, C other than 1 or 3; RSLF_ERR_UNSUPPORTED: V * U beyond 2^31 - 1. */
int rslf_apply_view_gains_dense(rslf_ctx* ctx, const float* d_in_vsuc, int elem, int V, int S, int U, int C, float hi,
                                const float* h_a_b, float* d_out_vsuc);
/* The joint statistic adds three channels' sums in one uint64, exact while 3 * V * U * 65535^2 < 2^64: every entry that takes
 * `joint` refuses joint != 0 with V * U beyond 1431699457 as RSLF_ERR_UNSUPPORTED (rslf_equalize_coefficients is not told V
 * and U: its caller keeps to the cap). */

/* Host EPIs as the reference holds them: h_epis[v] -> S rows of U*C values,
 * row_stride_bytes apart (cv::Mat::step).  u8: x * float(1/255) (dc.hpp:470).
 * f32: x * float(1/double(scale)); scale < 0 => the max over all EPIs
 * (dc.hpp:442-460, :474).  scale_used is nullable.
 * u16 (CV_16U): the reference's rule for every depth other than 8U, the f32 one
 * applied to float(x) (exact for ushort): the slab and scale_used are
 * bit-identical to the f32 upload of the same values with the same factor. */
int rslf_volume_upload_epis_f32(rslf_volume* vol, const float* const* h_epis, size_t row_stride_bytes,
                                float epi_scale_factor, float* scale_used);
int rslf_volume_upload_epis_u8(rslf_volume* vol, const uint8_t* const* h_epis, size_t row_stride_bytes);
int rslf_volume_upload_epis_u16(rslf_volume* vol, const uint16_t* const* h_epis, size_t row_stride_bytes,
                                float epi_scale_factor, float* scale_used);
/* Host image stack as read from disk, h_imgs[s] -> V rows of U*C values: the
 * input of rslf::build_epis_from_imgs (src/rslf_io.cpp:194-227); the
 * [s][v][u] -> [v][s][u] transposition happens on the device. */
int rslf_volume_upload_images_f32(rslf_volume* vol, const float* const* h_imgs, size_t row_stride_bytes,
                                  float epi_scale_factor, float* scale_used);
int rslf_volume_upload_images_u8(rslf_volume* vol, const uint8_t* const* h_imgs, size_t row_stride_bytes);
int rslf_volume_upload_images_u16(rslf_volume* vol, const uint16_t* const* h_imgs, size_t row_stride_bytes,
                                  float epi_scale_factor, float* scale_used);
/* The same with the two per-EPI options of rslf::build_epis_from_imgs (src/rslf_io.cpp:194-227, arguments `transpose`,
 * `rotate_180`): the EPI of scanline v is E[i][x] = h_imgs[i](v, x); transpose stores E^T -- the volume then has
 * S = image columns and U = number of images, h_imgs holds vol->U images of V rows x vol->S columns -- and
 * rotate_180 turns the (transposed) EPI by 180 degrees, i.e. reverses both of its axes. */
int rslf_volume_upload_images_xf_f32(rslf_volume* vol, const float* const* h_imgs, size_t row_stride_bytes,
                                     float epi_scale_factor, float* scale_used, int transpose, int rotate_180);
int rslf_volume_upload_images_xf_u8(rslf_volume* vol, const uint8_t* const* h_imgs, size_t row_stride_bytes,
                                    int transpose, int rotate_180);
int rslf_volume_upload_images_xf_u16(rslf_volume* vol, const uint16_t* const* h_imgs, size_t row_stride_bytes,
                                     float epi_scale_factor, float* scale_used, int transpose, int rotate_180);
/* Device-resident dense [V][S][U][C] float32 (already on this GPU). */
int rslf_volume_pack_device_f32(rslf_volume* vol, const float* d_vsuc, float epi_scale_factor, float* scale_used);

/* ---- the hot path, device pointers ------------------------------------ */
/* rslf::compute_1D_edge_confidence_pile -- core.hpp:279-287, impl :728-770
 * (per row :426-478).  d_Ce_vu [V][U] f32 is IN/OUT: the reference accumulates
 * into the caller's plane (src/rslf_depth_computation_core.cpp:10), pass zeros.
 * d_Ce_mask_vu [V][U] u8 out (0/255). */
int rslf_edge_confidence_pile(rslf_ctx* ctx, const rslf_volume* vol, int s, const rslf_params* p,
                              float* d_Ce_vu, uint8_t* d_Ce_mask_vu);

/* rslf::compute_1D_depth_epi_pile -- core.hpp:293-310, impl :772-893
 * (per EPI :480-661, selective median :663-718).
 *   d_dmin_vu/d_dmax_vu  [V][U] f32 per-pixel hypothesis range; both NULL =>
 *                        the scalars dmin/dmax (what dc.hpp:486-487 fills in)
 *   d_Ce_vu, d_Ce_mask_vu  in/out: a pixel whose best score is not above
 *                        raw_score_threshold gets C_e = 0, mask = 0 (:653-657)
 *   d_Cd_vu, d_depth_vu, d_rbar_vu  in/out, written only at scanned pixels;
 *                        d_rbar_vu is [V][U][C]; d_depth_vu is then REPLACED by
 *                        the selective median of itself (:881-892), 0 where the
 *                        edge mask is 0
 *   d_mask_vu            nullable in/out scan mask, AND-ed with the edge mask
 *                        in place (:510-511); NULL => edge mask alone (:513)
 *   d_idx_vu             nullable out, int32 argmax index d*, -1 if none
 *                        (not in the reference; the bit-exactness witness)
 *   d_score_vu           nullable out, score[d*]
 *   d_depth_raw_vu       nullable out, d_depth_vu before the median */
int rslf_depth_epi_pile(rslf_ctx* ctx, const rslf_volume* vol,
                        const float* d_dmin_vu, const float* d_dmax_vu, float dmin, float dmax,
                        int dim_d, int s_hat,
                        float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu, float* d_depth_vu,
                        float* d_rbar_vu, const rslf_params* p, uint8_t* d_mask_vu,
                        int32_t* d_idx_vu, float* d_score_vu, float* d_depth_raw_vu,
                        rslf_stats* stats);

/* rslf::compute_1D_depth_epi -- core.hpp:251-267, impl :480-661 -- for every EPI of the volume and
 * nothing else (no selective median): the first half of rslf_depth_epi_pile, same arguments, and all
 * the single-EPI class rslf::Depth1DComputer<T> needs. */
int rslf_depth_epi_scan(rslf_ctx* ctx, const rslf_volume* vol,
                        const float* d_dmin_vu, const float* d_dmax_vu, float dmin, float dmax,
                        int dim_d, int s_hat,
                        float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu, float* d_depth_vu,
                        float* d_rbar_vu, const rslf_params* p, uint8_t* d_mask_vu,
                        int32_t* d_idx_vu, float* d_score_vu, rslf_stats* stats);

/* rslf::Depth1DComputer<T>::run() -- include/rslf_depth_computation.hpp:325-371 with the
 * constructor's zero-filled outputs (:313-322): edge confidence and scan of each EPI on its own, no
 * median.  The reference's class holds one EPI; a volume of V EPIs is V independent instances. */
int rslf_depth1d_run(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, int s_hat,
                     const rslf_params* p,
                     float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu, float* d_depth_vu,
                     float* d_rbar_vu, int32_t* d_idx_vu, float* d_score_vu, rslf_stats* stats);

/* The optional last argument of compute_1D_depth_epi / _pile (a_K_r_m_rbar_(v_)s_u, core.hpp:266, :309; written at
 * :647-651): for every pixel that received a disparity, K(r - rbar)[:, d*] of its winning hypothesis, i.e. the
 * kernel values of the last mean-shift pass over the S views.  d_idx_vu is the arg-max plane a scan produced
 * (rslf_depth_epi_scan / rslf_depth_epi_pile with the same volume, ranges, dim_d, s_hat and parameters);
 * d_K_vsu is [V][S][U] (the reference's Vec<Mat> of V mats S x U).  Pixels with idx < 0 are left untouched, as
 * the reference leaves them.  Costs 1/dim_d of a scan. */
int rslf_kernel_columns_pile(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu,
                             float dmin, float dmax, int dim_d, int s_hat, const rslf_params* p,
                             const int32_t* d_idx_vu, float* d_K_vsu);

/* The scan's whole score matrix: what compute_1D_depth_epi leaves in the caller's BufferDepth1D::buf_scores_u_d
 * (core.hpp:616-625), from which it takes the arg max (:634) and C_d (:641) -- for the scanlines
 * [v_first, v_first + n_rows) of the volume.
 *   d_mask_vu       nullable, read-only, a full [V][U] plane: the pixels with a non-zero byte are scanned; NULL => every
 *                   pixel.  To reproduce the reference pass the mask a scan was ENTERED with (edge mask AND scan mask):
 *                   the reference writes a pixel's row before it tests raw_score_threshold.
 *   d_scores_vud    out, [n_rows][U][dim_d], d fastest: d_scores_vud[((v - v_first) * U + u) * dim_d + d] = score[d].
 *                   Rows of unscanned pixels are left untouched (as rslf_kernel_columns_pile leaves its columns).
 *   d_dmin_vu, d_dmax_vu   both NULL => the scalars; else the per-pixel [V][U] planes.
 * Nothing else is written: no C_e, mask, depth or C_d.  Arguments are checked as rslf_depth_epi_scan checks them, plus
 * the window; stats (nullable; waits) reports the pixels scanned and in scan_kernel the form that ran: RSLF_SCAN_REG for
 * the volumes the register scan takes, else RSLF_SCAN_GENERIC (also under the "force_scan" hook).  One device; not
 * inside an open sweep (it uses the context's pixel lists). */
int rslf_depth_epi_scores(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu,
                          float dmin, float dmax, int dim_d, int s_hat, const rslf_params* p,
                          const uint8_t* d_mask_vu, int v_first, int n_rows, float* d_scores_vud, rslf_stats* stats);
/* The same with the mask and the scores on the host.  The window goes through the context's staging buffer in passes
 * of as many scanlines as its budget holds (at least one; the "staging_kib" hook sets the budget); rows of unscanned
 * pixels are written 0, as the reference's zero-filled buffer holds them (core.hpp:167).  Synchronises. */
int rslf_depth_epi_scores_host(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu,
                               float dmin, float dmax, int dim_d, int s_hat, const rslf_params* p,
                               const uint8_t* h_mask_vu, int v_first, int n_rows, float* h_scores_vud, rslf_stats* stats);

/* The peaks of the score rows: per pixel the winner, a sub-grid disparity and the runner-up peak (the peak-ratio ambiguity
 * measure), computed on the device from the rows above.  Not in the reference; no existing output changes.
 * With s[0..D-1] a pixel's scores and [lo, hi] its range (the scalars, or its entries of the planes), every operation one
 * IEEE binary32 operation in the order written:
 *   candidates    j with (j == 0 || s[j] > s[j-1]) && (j == D-1 || s[j] >= s[j+1]): the first element of each local
 *                 maximum or plateau
 *   idx, score    i1 = the candidate with the largest score, the first on ties (the scan's arg max); s1 = s[i1]
 *   runner_*      i2 = the candidate with the largest score among the others, the first on ties (a later one as high as
 *                 the winner counts); s[i2]; -1 and 0 without another candidate
 *   disp          Dd + delta * step, with Dd = lo + ((float)i1 * (hi - lo)) / (float)(D-1) (the scan's grid value),
 *                 step = (hi - lo) / (float)(D-1), and delta = 0 at i1 == 0 or D-1, else with a = s[i1-1], c = s[i1+1]:
 *                 den2 = ((a + c) - (s1 + s1)) doubled by one addition, delta = den2 == 0 ? 0 : (a - c) / den2 clamped
 *                 to [-0.5, 0.5] -- the vertex of the parabola through the three points
 * A NaN score gives unspecified values (no fault).  Each of the five planes, [n_rows][U], may be NULL, not all of them. */
typedef struct rslf_peaks {
    int32_t* idx;
    float* score;
    float* disp;
    int32_t* runner_idx;
    float* runner_score;
} rslf_peaks;

/* The peaks of rows the caller holds: d_scores_vud is [n_rows][U][dim_d] as rslf_depth_epi_scores writes it for the
 * scanlines [v_first, v_first + n_rows); the mask (nullable) and the range planes (both or neither) are full [V][U]
 * planes, read at those scanlines.  Pixels whose mask byte is 0 are neither read nor written.  dim_d in [2, 2^24].
 * Queued on the context's stream; does not wait. */
int rslf_score_peaks(rslf_ctx* ctx, const float* d_scores_vud, int U, int dim_d, const float* d_dmin_vu, const float* d_dmax_vu,
                     float dmin, float dmax, const uint8_t* d_mask_vu, int v_first, int n_rows, const rslf_peaks* d_out);
/* Score rows and their peaks for a window of scanlines: arguments as rslf_depth_epi_scores, checked the same way.  The
 * rows go through the context's staging buffer in passes of as many scanlines as its budget holds (at least one; the
 * "staging_kib" hook sets the budget) and never leave the device.  d_out: device planes [n_rows][U]; pixels outside the
 * mask are left untouched.  Everything is queued on the context's stream; it waits only when stats is given.  One device;
 * not inside an open sweep (it uses the context's pixel lists; a sweep has rslf_sweep_peaks). */
int rslf_depth_epi_peaks(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu,
                         float dmin, float dmax, int dim_d, int s_hat, const rslf_params* p,
                         const uint8_t* d_mask_vu, int v_first, int n_rows, const rslf_peaks* d_out, rslf_stats* stats);
/* The same with the mask and the five planes on the host (the range planes stay device pointers, as in
 * rslf_depth_epi_scores_host).  Unscanned pixels get idx = runner_idx = -1 and the floats 0.  Synchronises. */
int rslf_depth_epi_peaks_host(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu,
                              float dmin, float dmax, int dim_d, int s_hat, const rslf_params* p,
                              const uint8_t* h_mask_vu, int v_first, int n_rows, const rslf_peaks* h_out, rslf_stats* stats);

/* rslf::selective_median_filter -- core.hpp:366-375, impl :663-718.
 * d_dst_vu must not alias d_src_vu; it is fully written (0 where mask is 0).
 * `size` = a_size: the window is width = (size - 1) / 2 pixels either side (:686), so an even size is the next smaller
 * odd window and 0 the 1 x 1 window; any size >= 0 runs (the report documents 11, report/rs_report.tex:388). */
int rslf_selective_median(rslf_ctx* ctx, const rslf_volume* vol, const float* d_src_vu, float* d_dst_vu,
                          int s_hat, int size, const uint8_t* d_mask_vu, float epsilon);

/* rslf::Depth1DComputer_pile<T>::run() -- include/rslf_depth_computation.hpp:513-565
 * with the output allocation of the constructor (:486-510): zero-fills the
 * outputs (the reference leaves C_e and C_d uninitialised, :501-504), s_hat < 0
 * or > S-1 => floor(S/2) (:490-498), then the two calls above, no scan mask. */
int rslf_depth1d_pile_run(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, int s_hat,
                          const rslf_params* p,
                          float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu, float* d_depth_vu,
                          float* d_rbar_vu, int32_t* d_idx_vu, float* d_score_vu, float* d_depth_raw_vu,
                          rslf_stats* stats);

/* ---- the hot path, host pointers (cv::Mat::data in / out) -------------- */
/* Same as rslf_depth1d_pile_run with host result planes: runs on the device,
 * copies back, synchronises.  Any output may be NULL. */
int rslf_depth1d_pile_run_host(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, int s_hat,
                               const rslf_params* p,
                               float* h_Ce_vu, uint8_t* h_Ce_mask_vu, float* h_Cd_vu, float* h_depth_vu,
                               float* h_rbar_vu, int32_t* h_idx_vu, float* h_score_vu, float* h_depth_raw_vu,
                               rslf_stats* stats);

/* ---- sub-grid disparities in the pile step ------------------------------ */
/* A scan's arg max moved off the hypothesis grid without a score row in memory.  Not in the reference; no existing entry
 * changes.  d_idx_vu is the arg-max plane a scan produced, d_score_vu (nullable) its score plane (rslf_depth_epi_scan /
 * rslf_depth_epi_pile with the same volume, ranges, dim_d, s_hat and parameters).  For every pixel with 0 <= idx < dim_d the
 * hypotheses idx - 1 and idx + 1 are scored again with the scan's arithmetic -- the scan's own bits, whichever kernel ran
 * it -- and, when no score plane is given, idx itself; with a, s1, c the three scores
 *   d_disp_vu    the `disp` of rslf_peaks above: the vertex of the parabola through the three points, clamped to half a
 *                step; the grid value at idx == 0, idx == dim_d - 1 and where den2 == 0.  It may be the scan's depth
 *                plane: nothing is read from it
 *   d_left_vu    nullable: a, written 0 at idx == 0
 *   d_right_vu   nullable: c, written 0 at idx == dim_d - 1
 * A pixel with idx < 0 (or >= dim_d) is left untouched in every output.  Costs 2 / dim_d of a generic scan (3 / dim_d
 * without the score plane).  Arguments are checked as rslf_kernel_columns_pile checks them; one launch, queued on the
 * context's stream, does not wait; it uses no context lists, so it is legal inside an open sweep. */
int rslf_subgrid_refine(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu,
                        float dmin, float dmax, int dim_d, int s_hat, const rslf_params* p,
                        const int32_t* d_idx_vu, const float* d_score_vu /*nullable*/, float* d_disp_vu,
                        float* d_left_vu /*nullable*/, float* d_right_vu /*nullable*/);

/* The entries above with a last argument `subgrid`.  0: exactly the namesake's launches and planes.  1: after the scan every
 * pixel with idx >= 0 has its disparity replaced by rslf_subgrid_refine's disp (the arg-max and score planes are the
 * caller's, or the context's own where NULL is passed), and the selective median, where the namesake has one, filters that
 * plane; d_depth_raw_vu holds the refined, unfiltered plane.  C_e, the mask, C_d, rbar, idx and score are bit for bit what
 * subgrid = 0 gives (rbar stays the grid winner's).  One device.  The 2-D sweep and fine-to-coarse have the mode as state of
 * an open sweep: rslf_sweep_subgrid and the *_sub entries below it. */
int rslf_depth_epi_pile_sub(rslf_ctx* ctx, const rslf_volume* vol,
                            const float* d_dmin_vu, const float* d_dmax_vu, float dmin, float dmax,
                            int dim_d, int s_hat,
                            float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu, float* d_depth_vu,
                            float* d_rbar_vu, const rslf_params* p, uint8_t* d_mask_vu,
                            int32_t* d_idx_vu, float* d_score_vu, float* d_depth_raw_vu,
                            rslf_stats* stats, int subgrid);
int rslf_depth_epi_scan_sub(rslf_ctx* ctx, const rslf_volume* vol,
                            const float* d_dmin_vu, const float* d_dmax_vu, float dmin, float dmax,
                            int dim_d, int s_hat,
                            float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu, float* d_depth_vu,
                            float* d_rbar_vu, const rslf_params* p, uint8_t* d_mask_vu,
                            int32_t* d_idx_vu, float* d_score_vu, rslf_stats* stats, int subgrid);
int rslf_depth1d_run_sub(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, int s_hat,
                         const rslf_params* p,
                         float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu, float* d_depth_vu,
                         float* d_rbar_vu, int32_t* d_idx_vu, float* d_score_vu, rslf_stats* stats, int subgrid);
int rslf_depth1d_pile_run_sub(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, int s_hat,
                              const rslf_params* p,
                              float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu, float* d_depth_vu,
                              float* d_rbar_vu, int32_t* d_idx_vu, float* d_score_vu, float* d_depth_raw_vu,
                              rslf_stats* stats, int subgrid);
int rslf_depth1d_pile_run_host_sub(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, int s_hat,
                                   const rslf_params* p,
                                   float* h_Ce_vu, uint8_t* h_Ce_mask_vu, float* h_Cd_vu, float* h_depth_vu,
                                   float* h_rbar_vu, int32_t* h_idx_vu, float* h_score_vu, float* h_depth_raw_vu,
                                   rslf_stats* stats, int subgrid);

/* ---- the hot path from host buffers, pipelined, over one or several devices --------------------------------- */
/* Depth1DComputer_pile<T>'s constructor + run() + result Mats (include/rslf_depth_computation.hpp:425-565) in ONE
 * call on host buffers: h_epis[v] is EPI v (S rows of U pixels, C channels interleaved, rows row_stride_bytes apart,
 * 0 = dense), the h_* planes are the caller's [V][U] result planes (any may be NULL).
 *
 * The V EPIs are cut into one contiguous block of scanlines per device of the rslf_multi (K1 and K2 are
 * independent per scanline, core.hpp:743-757 / :799-854; the median reads +-2 rows, core.hpp:686 -- those rows are
 * recomputed, not exchanged), every block into chunks, and per device the upload of chunk k+1, the kernels of chunk k
 * and the download of chunk k-1 overlap.  Each device's rows land directly at their offset in the caller's planes:
 * there is no collective.  The float input's default scale (epi_scale_factor < 0: the maximum over ALL EPIs,
 * dc.hpp:442-460) is taken once over the whole input, never per block.  Results are bit-identical to
 * rslf_volume_upload_epis_* + rslf_depth1d_pile_run_host on one device.
 *
 * devices may name the same GPU more than once (two workers on one GPU); NULL / 0 = device 0 alone. */
typedef struct rslf_multi rslf_multi;
int rslf_multi_create(const int* devices, int n_devices, rslf_multi** out);
int rslf_multi_destroy(rslf_multi* m);
int rslf_multi_device_count(const rslf_multi* m);
/* 1 if worker `from` can map worker `to`'s memory (hipDeviceCanAccessPeer) and the access has been enabled -- copies
 * between them then go device to device over xGMI; 0 if the copies stage through the host (still correct); 1 for two
 * workers on one GPU; <0 on a bad index.  rslf_multi_create enables peer access for every pair that allows it. */
int rslf_multi_peer_access(const rslf_multi* m, int from, int to);
int rslf_multi_set_chunk_rows(rslf_multi* m, int rows);   /* scanlines per chunk; 0 = automatic (about 8 chunks per device) */
int rslf_multi_depth1d_pile_f32(rslf_multi* m, const float* const* h_epis, size_t row_stride_bytes, int V, int S, int U, int C,
                                float epi_scale_factor, float dmin, float dmax, int dim_d, int s_hat, const rslf_params* p,
                                float* h_Ce_vu, uint8_t* h_Ce_mask_vu, float* h_Cd_vu, float* h_depth_vu, float* h_rbar_vu,
                                int32_t* h_idx_vu, float* h_score_vu, float* h_depth_raw_vu, rslf_stats* stats, float* scale_used);
/* Device-out form: the result planes live on device `out_device` (any device, one of the rslf_multi's or not); every
 * worker copies its rows to their place there with hipMemcpyPeerAsync -- point-to-point over xGMI, no collective and no
 * staging on the host.  Returns when the planes are complete. */
int rslf_multi_depth1d_pile_f32_dev(rslf_multi* m, const float* const* h_epis, size_t row_stride_bytes, int V, int S, int U, int C,
                                    float epi_scale_factor, float dmin, float dmax, int dim_d, int s_hat, const rslf_params* p,
                                    int out_device, float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu, float* d_depth_vu,
                                    float* d_rbar_vu, int32_t* d_idx_vu, float* d_score_vu, float* d_depth_raw_vu, rslf_stats* stats,
                                    float* scale_used);
int rslf_multi_depth1d_pile_u8(rslf_multi* m, const uint8_t* const* h_epis, size_t row_stride_bytes, int V, int S, int U, int C,
                               float dmin, float dmax, int dim_d, int s_hat, const rslf_params* p,
                               float* h_Ce_vu, uint8_t* h_Ce_mask_vu, float* h_Cd_vu, float* h_depth_vu, float* h_rbar_vu,
                               int32_t* h_idx_vu, float* h_score_vu, float* h_depth_raw_vu, rslf_stats* stats);
/* CV_16U EPIs: arguments as rslf_multi_depth1d_pile_f32 (the scale rule of rslf_volume_upload_epis_u16); results
 * bit-identical to the f32 form on the same values. */
int rslf_multi_depth1d_pile_u16(rslf_multi* m, const uint16_t* const* h_epis, size_t row_stride_bytes, int V, int S, int U, int C,
                                float epi_scale_factor, float dmin, float dmax, int dim_d, int s_hat, const rslf_params* p,
                                float* h_Ce_vu, uint8_t* h_Ce_mask_vu, float* h_Cd_vu, float* h_depth_vu, float* h_rbar_vu,
                                int32_t* h_idx_vu, float* h_score_vu, float* h_depth_raw_vu, rslf_stats* stats, float* scale_used);

/* ---- "next" row: the 2-D sweep over all views ------ */
/* Planes here are [S][V][U] (the reference's Vec<Mat> indexed by s, dc.hpp:208-215),
 * d_rbar_svu is [S][V][U][C]. */

/* rslf::compute_2D_edge_confidence -- core.hpp:323-330, impl :901-931: the pile edge
 * confidence for every view.  d_Ce_svu in/out (accumulates, pass zeros). */
int rslf_edge_confidence_2d(rslf_ctx* ctx, const rslf_volume* vol, const rslf_params* p,
                            float* d_Ce_svu, uint8_t* d_Ce_mask_svu);

/* rslf::compute_2D_depth_epi -- core.hpp:336-351, impl :933-1133 (default build: neither
 * _USE_DISP_CONFIDENCE_SCORE nor _USE_LINE_CONFIDENCE_SCORE, so propagation is gated by the edge
 * mask, :1099-1103).  Views are visited s_hat = floor(S/2), s_hat+1, s_hat-1, ... (:981-990); each
 * visit runs rslf_depth_epi_pile on the running mask (:1012-1028) and then propagates the
 * median-filtered disparities along their EPI lines into every view (:1088-1129).
 *   d_dmin_svu/d_dmax_svu  [S][V][U], both NULL => scalars dmin/dmax (dc.hpp:718-722)
 *   d_scan_mask_svu        nullable out: the running masks after the last visit
 *   stats->units           sums the units of all visits */
int rslf_depth_epi_2d(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu,
                      float dmin, float dmax, int dim_d,
                      float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu, float* d_depth_svu,
                      float* d_rbar_svu, const rslf_params* p, uint8_t* d_scan_mask_svu, rslf_stats* stats);

/* The sweep one visit at a time -- for callers that shard the scanlines of a sweep over devices (DESIGN.md
 * "Multi-GPU").  Scan and propagation are local to a scanline (core.hpp:1012-1028, :1088-1129) but the selective median
 * of a visit reads +-(size-1)/2 scanlines of the visited view's raw disparities and edge mask (core.hpp:686), which a
 * neighbouring device has just written: between rslf_sweep_visit_scan and rslf_sweep_visit_finish the caller brings
 * those rows of d_depth_svu[s_hat] and d_Ce_mask_svu[s_hat] up to date (a 2-row exchange with each neighbour).
 *   begin:  scanlines [v_lo, v_hi) of the volume are this device's own; the others are halo rows -- their running mask is
 *           cleared, so nothing is ever scanned or painted on them here.  (0, V) = an unsharded sweep.
 *   visits: in the reference's order, centre view outwards (core.hpp:981-990).
 *   end:    restores the context (call it with ok = 0 after a failed step); stats count the own scanlines only.
 * rslf_depth_epi_2d is exactly begin + (scan, finish) per view + end on (0, V). */
int rslf_sweep_begin(rslf_ctx* ctx, const rslf_volume* vol, const uint8_t* d_Ce_mask_svu, uint8_t* d_scan_mask_svu, int dim_d,
                     int v_lo, int v_hi);
int rslf_sweep_visit_scan(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu, float dmin,
                          float dmax, int dim_d, int s_hat, float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu,
                          float* d_depth_svu, float* d_rbar_svu, const rslf_params* p);
int rslf_sweep_visit_finish(rslf_ctx* ctx, const rslf_volume* vol, int s_hat, uint8_t* d_Ce_mask_svu, float* d_Cd_svu,
                            float* d_depth_svu, float* d_rbar_svu, const rslf_params* p);
int rslf_sweep_end(rslf_ctx* ctx, int ok, int dim_d, rslf_stats* stats);

/* rslf::Depth2DComputer<T>::run() -- include/rslf_depth_computation.hpp:748-805 with the
 * constructor's output allocation (:718-750): zero-fills the outputs, then the two calls above. */
int rslf_depth2d_run(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                     float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu, float* d_depth_svu,
                     float* d_rbar_svu, uint8_t* d_scan_mask_svu, rslf_stats* stats);

/* ---- the line confidence C_l of the 2-D sweep (K7) ------------------------ */
/* The reference's third criterion, C_l = sum_s C_e(s) K(r_s - rbar) / sum_s K(r_s - rbar) along a pixel's EPI line
 * (report/rs_report.tex:700-704), as compute_2D_depth_epi computes it under -D_USE_LINE_CONFIDENCE_SCORE
 * (core.hpp:1032-1081) and carries it along the propagation (:1122-1124).  The places that would GATE on it
 * (core.hpp:1099, dc.hpp:841, :881, :903) sit behind an `#elseif` typo inside a skipped group and are never compiled:
 * OFF       the default build: no line confidence, exactly the launches of rslf_depth_epi_2d.
 * AS_BUILT  what the macro compiles to: the planes are computed and carried, the gate stays the edge mask, every other
 *           plane is bit for bit the OFF result.
 * GATE      what the `#elseif` branches say: a pixel is a source of the propagation iff C_l > (float)line_score_threshold
 *           (no edge-mask test, as core.hpp:1100 has none).
 * With use_disp_confidence_score the #ifdef chain gives C_d the gate in every mode; C_l is still computed and carried. */
#define RSLF_LINE_CONF_OFF       0
#define RSLF_LINE_CONF_AS_BUILT  1
#define RSLF_LINE_CONF_GATE      2

/* core.hpp:1054-1079 for one visited view on caller planes: for every pixel of d_Ce_mask_vu ([V][U]),
 *   I = (float)((double)(s_hat - s) * (double)depth + (double)u)  (:1058, one gemm; no slope_factor, as written)
 *   E = max(lerp of d_Ce_svu[s][v][.] at I, 0), NaN outside [0, U-1] -> 0  (:1069-1071, interp.hpp:155-193)
 *   d_Cl_vu = sum_s E K / sum_s K, float sums with s ascending, x / 0 -> 0  (:1074-1079)
 * with K = d_K_vsu [V][S][U].  d_Ce_svu is [S][V][U], d_depth_vu [V][U].  Pixels outside the mask keep what d_Cl_vu held.
 * A disparity that is NaN or sends I beyond the int range neither faults nor hangs; what it gives is unspecified. */
int rslf_line_confidence_pile(rslf_ctx* ctx, int V, int S, int U, int s_hat, const float* d_Ce_svu, const float* d_K_vsu,
                              const float* d_depth_vu, const uint8_t* d_Ce_mask_vu, float* d_Cl_vu);

/* Line confidence is state of an open sweep: valid between rslf_sweep_begin and the first visit, cleared by
 * rslf_sweep_end.  mode: RSLF_LINE_CONF_*; d_Cl_svu: the [S][V][U] plane the visits fill and the propagation paints
 * (a_line_confidence_s_v_u, core.hpp:345; dc.hpp:737 leaves it uninitialised: pass zeros), required for mode >= 1.
 * Sizes the sweep-long K(r - rbar) columns [V][S][U] (core.hpp:975-979; zero-filled here, uninitialised there) and the
 * visits' arg-max plane in the context's grow-only scratch: no visit allocates.  A visit is then
 *   AS_BUILT  scan -> median + claims -> K7 -> apply
 *   GATE      scan -> median -> K7 -> median + claims gated by C_l -> apply  (with use_disp_confidence_score, where C_d
 *             gates: the AS_BUILT order)
 * RSLF_ERR_INVALID_ARG: a mode outside 0..2, a NULL plane with mode >= 1, a call outside that window. */
int rslf_sweep_line_confidence(rslf_ctx* ctx, const rslf_volume* vol, int mode, float* d_Cl_svu);

/* rslf_depth_epi_2d, rslf_depth2d_run and rslf_depth2d_run_host with the reference's extra argument
 * a_line_confidence_s_v_u (core.hpp:345, handed over at dc.hpp:791-792; allocated at dc.hpp:721-738): the existing
 * signature plus line_mode (RSLF_LINE_CONF_*) and the [S][V][U] plane (NULL allowed with mode 0, which is the plain
 * entry).  rslf_depth2d_run_lc also zero-fills d_Cl_svu (dc.hpp:737 leaves it uninitialised). */
int rslf_depth_epi_2d_lc(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu,
                         float dmin, float dmax, int dim_d,
                         float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu, float* d_depth_svu,
                         float* d_rbar_svu, const rslf_params* p, uint8_t* d_scan_mask_svu, rslf_stats* stats,
                         int line_mode, float* d_Cl_svu);
int rslf_depth2d_run_lc(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                        float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu, float* d_depth_svu,
                        float* d_rbar_svu, uint8_t* d_scan_mask_svu, rslf_stats* stats, int line_mode, float* d_Cl_svu);
int rslf_depth2d_run_host_lc(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                             float* h_Ce_svu, uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu,
                             float* h_rbar_svu, rslf_stats* stats, int line_mode, float* h_Cl_svu);

/* ---- sub-grid disparities in the 2-D sweep (K9 inside a visit) ------------- */
/* The sub-grid mode is state of an open sweep, as line confidence is: valid between rslf_sweep_begin and the first visit,
 * cleared by rslf_sweep_end.  on = 1 sizes the visits' arg-max and score planes in the context's grow-only scratch (with
 * line confidence on, the scan writes ONE arg-max plane for K7 and K9): no visit allocates.  A visit is then
 *   scan (also writes idx and score) -> refinement -> the rest of the visit as without the mode
 * The refinement is queued at the end of rslf_sweep_visit_scan, in place on the view's raw depth plane: every pixel this
 * visit scanned and accepted (idx >= 0) gets rslf_subgrid_refine's disp; pixels painted by earlier visits keep the refined
 * value they were painted with.  The median, the claims' target columns u + round(d * (s_hat - s) * slope), the apply pass
 * and K7's positions then read refined floats.  rbar and the K columns stay the grid winner's; C_d, C_e and the masks are
 * what the scan wrote.  A visit whose scan took the packed list of the previous apply pass refines over that list
 * (k9_subgrid_refine_list, lane = entry); every other visit -- the first, "force_packed" = 0, planes beyond INT32_MAX pixels,
 * "subgrid_list" = 0 -- over the whole plane; the bits are the same.  With the mode off every entry queues the launches and
 * writes the bits it always did.  Between the visits of a sweep in the mode, the pile step's *_sub entries with NULL arg-max or
 * score planes are not supported: they would take the context's own planes, which are the visits'.
 * RSLF_ERR_INVALID_ARG: on outside 0..1, a call outside that window; nothing is launched. */
int rslf_sweep_subgrid(rslf_ctx* ctx, const rslf_volume* vol, int on);

/* The _lc entries with a last argument `subgrid`: 1 runs every visit in the mode, 0 is the _lc entry, launch for launch.  One
 * device: the multi-device forms (rslf_multi_*) have no such mode. */
int rslf_depth_epi_2d_sub(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu,
                          float dmin, float dmax, int dim_d,
                          float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu, float* d_depth_svu,
                          float* d_rbar_svu, const rslf_params* p, uint8_t* d_scan_mask_svu, rslf_stats* stats,
                          int line_mode, float* d_Cl_svu, int subgrid);
int rslf_depth2d_run_sub(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                         float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu, float* d_depth_svu,
                         float* d_rbar_svu, uint8_t* d_scan_mask_svu, rslf_stats* stats, int line_mode, float* d_Cl_svu,
                         int subgrid);
int rslf_depth2d_run_host_sub(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                              float* h_Ce_svu, uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu,
                              float* h_rbar_svu, rslf_stats* stats, int line_mode, float* h_Cl_svu, int subgrid);

/* ---- runner-up peaks in the 2-D sweep (K10 inside a visit) ----------------- */
/* The peaks mode is a third state of an open sweep, beside line confidence and the sub-grid mode: valid between
 * rslf_sweep_begin and the first visit, cleared by rslf_sweep_end.  Not in the reference; it changes no other plane.
 * d_out_svu: four caller planes [S][V][U] on the device -- idx, score, runner_idx, runner_score, whose meaning is exactly
 * that of rslf_peaks' fields of the same names above; each may be NULL, not all four.  `disp` is ignored by the visits and
 * must be NULL: the sub-grid mode already puts that value in the depth plane.  d_out_svu = NULL switches the mode off again.
 * Setting the mode sizes everything its visits use in the context's grow-only scratch: no visit allocates.  A visit is then
 *   scan (also writes idx and the winner's score: one arg-max plane for all three modes) -> sub-grid refinement if on ->
 *   peaks -> the rest of the visit as without the mode
 * The step is queued at the end of rslf_sweep_visit_scan.  A pixel gets its four values one of two ways:
 *   - a visit scanned and accepted it (the visit's arg-max plane has idx >= 0): the peaks of its own score row, every score
 *     the scan's own bits -- idx and score equal the scan's arg max and its score bit for bit;
 *   - a visit paints it: it takes its source's four values in the apply pass, as C_d and C_l are carried.
 * Every other pixel keeps what the caller put there (rslf_depth_epi_2d_pk fills nothing; the _run entries below fill
 * idx = runner_idx = -1 and the floats 0 first, as rslf_depth_epi_peaks_host does for unscanned pixels).
 * No score row is kept.  A visit whose scan took the packed list of the previous apply pass takes the list form
 * (k10_peaks_list: a wave per list entry, lanes = hypotheses in rounds of 64, each lane scoring its own hypothesis with the
 * generic scan's operations in their order, the peak rule across the lanes); every other visit -- the first,
 * "force_packed" = 0, planes beyond INT32_MAX pixels, "peaks_list" = 0 -- the dense form: the score rows of the plane,
 * window by window through the context's staging buffer (the "staging_kib" hook sets the budget), reduced by the kernel of
 * rslf_score_peaks under the mask "this visit's idx >= 0", on pixel lists of the step's own -- the sweep's packed list and
 * its length are read, never written.  The bits are the same; the cost is not: the list form pays a wave per pixel in the generic
 * per-hypothesis arithmetic, which wins where the later visits scan a few pixels per scanline (the usual sweep) and loses to
 * the dense form where they still scan a large share of a view -- on a 960 x 540 field of 100 views whose later visits scan a
 * quarter of a view each, 1679 ms against 483 ms (profiles/r16_sweep_peaks.md); set "peaks_list" = 0 for such fields.  The
 * form is chosen on the host, which does not know the list's length.  Line confidence modes 0 / 1 / 2 and the sub-grid mode combine
 * with the mode: it reads planes they write and writes none of theirs.  With the mode off every entry queues the launches
 * and writes the bits it always did.  One device; a kept fine-to-coarse run has the mode per level (rslf_f2c_run_host_pk), the
 * host-planes pyramid entries and the multi-device forms have none.
 * RSLF_ERR_INVALID_ARG: a call outside that window, a non-NULL disp, four NULL planes, a sweep begun with dim_d above 2^24
 * (the limit of rslf_score_peaks); nothing is launched.  The _pk entries below return the same for the same causes. */
int rslf_sweep_peaks(rslf_ctx* ctx, const rslf_volume* vol, const rslf_peaks* d_out_svu);

/* The _sub entries with a last argument: the four planes (device pointers; for rslf_depth2d_run_host_pk host planes
 * [S][V][U]).  NULL is the _sub entry, launch for launch. */
int rslf_depth_epi_2d_pk(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu,
                         float dmin, float dmax, int dim_d,
                         float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu, float* d_depth_svu,
                         float* d_rbar_svu, const rslf_params* p, uint8_t* d_scan_mask_svu, rslf_stats* stats,
                         int line_mode, float* d_Cl_svu, int subgrid, const rslf_peaks* d_pk_svu);
int rslf_depth2d_run_pk(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                        float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu, float* d_depth_svu,
                        float* d_rbar_svu, uint8_t* d_scan_mask_svu, rslf_stats* stats, int line_mode, float* d_Cl_svu,
                        int subgrid, const rslf_peaks* d_pk_svu);
int rslf_depth2d_run_host_pk(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                             float* h_Ce_svu, uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu,
                             float* h_rbar_svu, rslf_stats* stats, int line_mode, float* h_Cl_svu, int subgrid,
                             const rslf_peaks* h_pk_svu);

/* ---- the sweep gate: ambiguous pixels withheld from propagation by peak ratio ---- */
/* A fourth state of an open sweep, on top of the peaks mode with ALL FOUR planes given: valid between rslf_sweep_peaks and
 * the first visit; cleared by rslf_sweep_end and by every later call of rslf_sweep_peaks (which is how the mode is switched
 * off).  ratio = r in (0, 1]; 0 switches the gate off again.  Not in the reference, which has two gates of the same shape
 * (core.hpp:1097-1103: C_d > par_disp_score_threshold, and in line mode 2 C_l > par_line_score_threshold); this is a third.
 *
 * THE RULE.  In visit s_hat, pixel (v, u) is a propagation source only if
 *   1. it passes the gate it passes without the ratio: the edge mask, or C_d with use_disp_confidence_score, or C_l in line
 *      mode 2; and
 *   2. it is not ambiguous: NOT (idx >= 0 && runner_idx >= 0 && runner_score > r * score), the product one binary32
 *      multiply, the four values read from the peaks planes at (s_hat, v, u) -- the predicate of a kept pyramid's validity
 *      by uniqueness (rslf_f2c_run_host_pk below), one statement in the source for both.
 * The values exist at that moment: a pixel this visit scanned got them from the peaks step rslf_sweep_visit_scan queues; a
 * pixel painted earlier carries its source's.  A withheld source makes NO claim, the one on itself (s == s_hat,
 * core.hpp:1119-1121) included -- exactly what happens to a pixel the C_d or C_l gate withholds today:
 *   - its depth plane keeps the raw scan value, not the median;
 *   - it stays in the running mask (scan_mask differs from the ungated sweep's);
 *   - a later visit's unambiguous source whose line passes through it and whose radiance matches may still paint it: it
 *     then takes that source's disparity, C_d, C_l and peaks;
 *   - the pixels it would have painted stay in their views' running masks and are scanned in their own visits.
 * r = 1 withholds nothing (a runner-up never scores above its winner: the bits of the plain peaks-mode sweep).  A NaN score
 * compares false: never ambiguous.  The line modes, use_disp_confidence_score, the sub-grid mode, per-pixel ranges, every
 * median window and the hooks ("force_packed", "peaks_list", "subgrid_list", "claim_skip", "staging_kib") combine with the
 * gate unchanged: it only narrows the set of sources.  With the ratio off every entry queues the launches and writes the
 * bits it always did; with it on, a visit's median + claims launch is k34_median_claim_gated, which loads the pixel's four
 * values (16 bytes a pixel, coalesced) and counts the withheld sources -- pixels that pass 1 and fail 2, summed over the
 * visits of the sweep -- with one atomic per wave.  Setting the ratio sizes the counter in the context's grow-only scratch
 * and zeroes it on the stream: no visit allocates.  One device; the multi-device entries have no such mode.
 * RSLF_ERR_INVALID_ARG with the cause in rslf_last_error(), nothing launched: a ratio below 0, above 1 or NaN; a call
 * outside that window; a ratio above 0 while the peaks mode is off; a NULL among the four planes. */
int rslf_sweep_propagation_ratio(rslf_ctx* ctx, const rslf_volume* vol, float ratio);
/* The withheld sources of the last sweep that ended with ok = 1 on this context: 0 if it had no ratio.  Synchronises the
 * context's stream.  RSLF_ERR_INVALID_ARG while a sweep is open. */
int rslf_sweep_withheld(rslf_ctx* ctx, unsigned long long* n);

/* The _pk entries with a last argument: the ratio.  0 is the _pk entry, launch for launch; above 0 it needs d_pk_svu with
 * four planes, refused before anything is queued otherwise. */
int rslf_depth_epi_2d_pr(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu,
                         float dmin, float dmax, int dim_d,
                         float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu, float* d_depth_svu,
                         float* d_rbar_svu, const rslf_params* p, uint8_t* d_scan_mask_svu, rslf_stats* stats,
                         int line_mode, float* d_Cl_svu, int subgrid, const rslf_peaks* d_pk_svu, float propagation_ratio);
int rslf_depth2d_run_pr(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                        float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu, float* d_depth_svu,
                        float* d_rbar_svu, uint8_t* d_scan_mask_svu, rslf_stats* stats, int line_mode, float* d_Cl_svu,
                        int subgrid, const rslf_peaks* d_pk_svu, float propagation_ratio);
int rslf_depth2d_run_host_pr(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                             float* h_Ce_svu, uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu,
                             float* h_rbar_svu, rslf_stats* stats, int line_mode, float* h_Cl_svu, int subgrid,
                             const rslf_peaks* h_pk_svu, float propagation_ratio);

/* ---- "next" row: fine-to-coarse ---------------------- */
/* rslf::FineToCoarse<T> (include/rslf_fine_to_coarse.hpp:26-81) is a host-side loop over pyramid
 * levels, each a Depth2DComputer (rslf_depth2d_run / rslf_depth_epi_2d above).  These are the pieces
 * between the levels; the loop itself lives in the host wrapper (depth.py: FineToCoarse).  Raw
 * (un-normalised) volumes here are dense float32 [V][S][U][C] on the device; uchar light fields keep uchar
 * arithmetic through the pyramid (rslf_downsample_epis_u8), as the reference's CV_8U Mats do. */

/* Level dimensions of cv::resize(0.5, 0.5): cvRound(V/2), cvRound(U/2) (ties to even). */
int rslf_f2c_level_dims(int V, int U, int* V2, int* U2);
/* rslf::downsample_EPIs -- src/rslf_fine_to_coarse_core.cpp:14-60: per view, cv::GaussianBlur(7x7,
 * sigma 0, BORDER_REFLECT) then cv::resize(0.5, 0.5, INTER_LINEAR).  d_out_vsuc is [V2][S][U2][C]. */
int rslf_downsample_epis_f32(rslf_ctx* ctx, const float* d_in_vsuc, int V, int S, int U, int C, float* d_out_vsuc);
/* The same for CV_8U light fields, in uchar arithmetic as the reference runs it (its Mats keep the input's type):
 * d_in / d_out hold uchar levels 0..255 as float32.  GaussianBlur on 8U = exact integer convolution (the taps are
 * exact in 8 fractional bits) rounded half up once -- the result of both 8U paths of OpenCV 3.4 (<= 3.4.0 8-bit
 * fixed-point filter, >= 3.4.1 ufixedpoint16); resize = INTER_AREA's (sum + 2) >> 2. */
int rslf_downsample_epis_u8(rslf_ctx* ctx, const float* d_in_vsuc, int V, int S, int U, int C, float* d_out_vsuc);
/* The same for CV_16U light fields (ushort levels 0..65535 as float32), as OpenCV 3.4 runs it without IPP: GaussianBlur =
 * sepFilter2D with the float kernel and a float buffer -- the row pass of rslf_downsample_epis_f32 (exact on ushort), its
 * column pass (centre tap, then k[j] * (S[y+j] + S[y-j])) rounded by saturate_cast<ushort> (cvRound, ties to even,
 * clamped to [0, 65535]); resize = INTER_AREA's (sum + 2) >> 2, cvRound((float)sum / count) at an odd border. */
int rslf_downsample_epis_u16(rslf_ctx* ctx, const float* d_in_vsuc, int V, int S, int U, int C, float* d_out_vsuc);
/* max over a device buffer: the per-level epi_scale_factor of Depth2DComputer's constructor
 * (include/rslf_depth_computation.hpp:671-690).  Synchronises. */
int rslf_device_max_f32(rslf_ctx* ctx, const float* d_values, size_t n, float* h_max);   /* returns the value: waits */
/* The three helpers below enqueue on the context's stream and return, like every device entry point. */
/* FineToCoarse::run(), bound tightening -- include/rslf_fine_to_coarse.hpp:171-299: d_dmin/d_dmax of
 * the coarser level ([S][V_down][U_down], in/out) from the finer level's disparities and validity. */
int rslf_f2c_tighten_bounds(rslf_ctx* ctx, const float* d_depth_up_svu, const uint8_t* d_valid_up_svu, int S, int V_up,
                            int U_up, float* d_dmin_down_svu, float* d_dmax_down_svu, int V_down, int U_down);
/* rslf::fuse_disp_maps -- src/rslf_fine_to_coarse_core.cpp:69-135, all views at once.
 * d_disp[p] / d_valid[p]: level p planes [S][Vp[p]][Up[p]] (p = 0 finest); outputs [S][Vp[0]][Up[0]]. */
int rslf_f2c_fuse(rslf_ctx* ctx, const float* const* d_disp, const uint8_t* const* d_valid, const int* Vp, const int* Up,
                  int P, int S, float* d_out_map_svu, uint8_t* d_out_valid_svu);

/* ---- the rows around the path, host pointers --------------------------- */
/* rslf::Depth2DComputer<T>::run() with host result planes ([S][V][U], rbar [S][V][U][C]; any may be NULL). */
int rslf_depth2d_run_host(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                          float* h_Ce_svu, uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu,
                          float* h_rbar_svu, rslf_stats* stats);

/* rslf::FineToCoarse<T>: constructor + run() + get_results() -- include/rslf_fine_to_coarse.hpp:103-324 --
 * from the reference's Vec<Mat> (h_epis[v] -> S rows of U*C values, row_stride_bytes apart; is_u8
 * selects uchar input).  The whole pyramid loop runs inside the library.
 *   h_out_map_svu / h_out_valid_svu  [S][V][U] fused disparity map and validity at the finest scale
 *   n_levels (nullable)              pyramid depth that was built
 *   stats->units                     sums every visit of every level */
int rslf_fine_to_coarse_run_host(rslf_ctx* ctx, const void* const* h_epis, int is_u8, int V, int S, int U, int C,
                                 size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                 const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                 float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats);
/* The same from CV_16U EPIs: the pyramid keeps ushort levels (rslf_downsample_epis_u16) and every level is normalised by
 * its own max, or by epi_scale_factor when that is >= 0 (dc.hpp:671-705). */
int rslf_fine_to_coarse_run_host_u16(rslf_ctx* ctx, const uint16_t* const* h_epis, int V, int S, int U, int C,
                                     size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                     const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                     float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats);

/* Fine-to-coarse with the line confidence (the -D_USE_LINE_CONFIDENCE_SCORE build of FineToCoarse<T>): every level's
 * sweep runs in line_mode (RSLF_LINE_CONF_*) with a zero-filled [S][V_p][U_p] C_l plane of its own, and each level's
 * validity -- which tightens the next level's ranges (rslf_fine_to_coarse.hpp:185-186) and feeds the fusion (:312) -- is
 * get_valid_depths_mask_s_v_u (dc.hpp:893-915):
 *   accept_all (the last level, when asked to)              everything (C_e > -1)
 *   RSLF_LINE_CONF_GATE without use_disp_confidence_score   C_l > (float)line_score_threshold  (:903-904)
 *   otherwise                                               C_e > (float)edge_score_threshold
 * (the RSLF_F2C_VALID_COMPAT table: under use_disp_confidence_score it reads C_e, not C_d; the whole chain of :893-915, C_d
 * included, is RSLF_F2C_VALID_REFERENCE of rslf_f2c_run_host below).  AS_BUILT changes nothing but the existence of the
 * C_l planes.  OFF with levels_out NULL queues exactly the launches of rslf_fine_to_coarse_run_host, which is that call.
 *
 * levels_out (nullable): host copies of every level's planes, finest first.  Each member is NULL (not wanted) or an array
 * of `capacity` host pointers, entry l NULL or room for [S][Vp[l]][Up[l]] values; the level sizes come from
 * rslf_f2c_pyramid_dims.  h_Cl_svu is filled in modes AS_BUILT and GATE only.
 * RSLF_ERR_INVALID_ARG, before anything is queued: a mode outside 0..2, a capacity below the pyramid depth. */
typedef struct rslf_f2c_levels_out {
    int capacity;            /* entries of each array below */
    float** h_depth_svu;     /* the level's disparities */
    uint8_t** h_valid_svu;   /* its validity mask, 0 / 255 */
    float** h_Cl_svu;        /* its line confidence */
    float** h_Ce_svu;        /* its edge confidence */
} rslf_f2c_levels_out;
/* The level sizes FineToCoarse's constructor builds (rslf_fine_to_coarse.hpp:130-154), finest first, into Vp / Up
 * [capacity], and their count into n_levels (0: the field is not larger than _MIN_SPATIAL_DIM).  capacity 0 (Vp / Up may
 * be NULL) asks for the count alone; a capacity in between is RSLF_ERR_INVALID_ARG. */
int rslf_f2c_pyramid_dims(int V, int U, int max_pyr_depth, int* Vp, int* Up, int capacity, int* n_levels);
int rslf_fine_to_coarse_run_host_lc(rslf_ctx* ctx, const void* const* h_epis, int is_u8, int V, int S, int U, int C,
                                    size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                    const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                    float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats,
                                    int line_mode, const rslf_f2c_levels_out* levels_out);
int rslf_fine_to_coarse_run_host_u16_lc(rslf_ctx* ctx, const uint16_t* const* h_epis, int V, int S, int U, int C,
                                        size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                        const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                        float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats,
                                        int line_mode, const rslf_f2c_levels_out* levels_out);

/* ---- fine-to-coarse kept on the device: a finished run as an object, its pictures rendered there ------------------ */
/* rslf_f2c_run is what FineToCoarse<T> is after run(): every level's Depth2DComputer results and the fused maps, held on ONE
 * device.  The getters of include/rslf_fine_to_coarse.hpp:325-519 then render from it (3 bytes per pixel leave the device)
 * and nothing is uploaded or computed a second time.  The object is bound to its device, not to the context that made it:
 * like a volume it may outlive that context, and it may be read and rendered through any context of the same device. */
typedef struct rslf_f2c_run rslf_f2c_run;

#define RSLF_ELEM_F32 0   /* the element type of host EPIs: CV_32F, */
#define RSLF_ELEM_U8  1   /* CV_8U, */
#define RSLF_ELEM_U16 2   /* CV_16U */

/* get_valid_depths_mask_s_v_u (dc.hpp:893-915) of every level -- the next level's ranges and the fusion:
 * COMPAT     the table of rslf_fine_to_coarse_run_host_lc above, what every other entry computes.
 * REFERENCE  the whole #ifdef chain: accept_all -> everything; else use_disp_confidence_score -> C_d > (float)
 *            disp_score_threshold (:902); else RSLF_LINE_CONF_GATE -> C_l > (float)line_score_threshold (:904); else
 *            C_e > (float)edge_score_threshold (:906).  The two differ under use_disp_confidence_score alone. */
#define RSLF_F2C_VALID_COMPAT    0
#define RSLF_F2C_VALID_REFERENCE 1

/* The planes of a kept run, [S][V_l][U_l] of level l (float32; VALID and FUSED_VALID bytes 0 / 255).  The fused planes are
 * at the finest size and are asked for with level 0.  CL is held in modes AS_BUILT and GATE only.  (Planes 7 .. 15: the peak
 * planes of rslf_f2c_run_host_pk below.) */
#define RSLF_F2C_PLANE_DEPTH       0
#define RSLF_F2C_PLANE_VALID       1
#define RSLF_F2C_PLANE_CE          2
#define RSLF_F2C_PLANE_CD          3
#define RSLF_F2C_PLANE_CL          4
#define RSLF_F2C_PLANE_FUSED_MAP   5
#define RSLF_F2C_PLANE_FUSED_VALID 6

#define RSLF_F2C_MAX_LEVELS 32   /* no pyramid is deeper: every level halves both sides of an int-sized field */
typedef struct rslf_f2c_run_desc {
    int n_levels;                                 /* pyramid depth */
    int S, C;                                     /* views, channels */
    int device;                                   /* the device that holds the run */
    int elem;                                     /* RSLF_ELEM_* of the EPIs it was made from */
    int line_mode;                                /* RSLF_LINE_CONF_* of every level's sweep */
    int validity_rule;                            /* RSLF_F2C_VALID_* */
    int keep_volumes;                             /* 1: every level's normalised volume is held */
    unsigned planes_held;                         /* bit (1 << RSLF_F2C_PLANE_*) set for every plane kind held */
    int V[RSLF_F2C_MAX_LEVELS];                   /* level sizes, finest first */
    int U[RSLF_F2C_MAX_LEVELS];
    float epi_scale_factor[RSLF_F2C_MAX_LEVELS];  /* as used: 255 for CV_8U, else the given factor or the level's own max */
    size_t device_bytes;                          /* what the object holds on the device */
} rslf_f2c_run_desc;

/* FineToCoarse<T>'s constructor + run() (rslf_fine_to_coarse.hpp:103-299) and the fusion of get_results() (:302-324) from
 * host EPIs (arguments as rslf_fine_to_coarse_run_host_lc; elem: RSLF_ELEM_*), kept: the level loop is the one of the
 * entries above, with an owner that keeps what they free.  Per level, finest first, the run holds the disparities, the
 * validity, C_e, C_d, C_l in modes 1 and 2 and -- with keep_volumes != 0 -- the normalised volume its sweep ran on; and the
 * fused map and fused validity.  Returns when the run is complete.  stats: nullable, as rslf_fine_to_coarse_run_host's.
 * On any failure *run is NULL and nothing stays allocated. */
int rslf_f2c_run_host(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C, size_t row_stride_bytes,
                      float d_min, float d_max, int dim_d, float epi_scale_factor, const rslf_params* p, int max_pyr_depth,
                      int accept_all_last_scale, int line_mode, int validity_rule, int keep_volumes, rslf_f2c_run** run,
                      rslf_stats* stats);
/* Fine-to-coarse with every level's sweep in the sub-grid mode (rslf_sweep_subgrid), through the one level loop: the bound
 * tightening, the validity rules and the fusion are untouched and receive off-grid disparities; coarser levels refine inside
 * their per-pixel ranges (lo == hi included: the refined value is lo).  subgrid = 0 is the namesake, launch for launch.
 * rslf_fine_to_coarse_run_host_sub: rslf_fine_to_coarse_run_host_lc's arguments with elem (RSLF_ELEM_*) in place of is_u8 --
 * so it has no u16 twin -- plus subgrid.  rslf_f2c_run_host_sub: rslf_f2c_run_host plus subgrid; rslf_f2c_run_subgrid reads
 * it back from a kept run (0 or 1; rslf_f2c_run_desc keeps its size).  One device. */
int rslf_fine_to_coarse_run_host_sub(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C,
                                     size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                     const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                     float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats,
                                     int line_mode, const rslf_f2c_levels_out* levels_out, int subgrid);
int rslf_f2c_run_host_sub(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C, size_t row_stride_bytes,
                          float d_min, float d_max, int dim_d, float epi_scale_factor, const rslf_params* p, int max_pyr_depth,
                          int accept_all_last_scale, int line_mode, int validity_rule, int keep_volumes, rslf_f2c_run** run,
                          rslf_stats* stats, int subgrid);
int rslf_f2c_run_subgrid(const rslf_f2c_run* run);
int rslf_f2c_run_destroy(rslf_f2c_run* run);   /* NULL is RSLF_OK; waits for the device */
int rslf_f2c_run_describe(const rslf_f2c_run* run, rslf_f2c_run_desc* out);
/* One plane (which: RSLF_F2C_PLANE_*) of one level into the caller's memory: a device pointer on the run's device, or with
 * dst_on_host != 0 a host pointer (the call then waits).  stream_ctx (nullable): a context of the run's device whose stream
 * the copy is queued on; NULL copies on the default stream and waits.  A plane that is not held, a level outside the
 * pyramid, a fused plane asked for with level != 0: RSLF_ERR_INVALID_ARG. */
int rslf_f2c_run_copy(const rslf_f2c_run* run, int level, int which, void* dst, int dst_on_host, rslf_ctx* stream_ctx);
/* Level `level`'s normalised volume, for rslf_volume_describe: owned by the run, gone with it.  RSLF_ERR_INVALID_ARG
 * without kept volumes.  (The render entries below take the run itself: rslf_render_planes wants a volume of its context.) */
int rslf_f2c_run_volume(const rslf_f2c_run* run, int level, const rslf_volume** out);

/* The three coloured getters, rendered on ctx (any context of the run's device) from the kept planes; pictures [..][3] uint8
 * BGR into device memory, or host memory in the _host forms (which wait).  saturate != 0: ImageConverter_uchar::fit's 2 % /
 * 98 % quantiles, else min and mean + 12 std.  The shadow cut follows the run's cut_shadows / shadow_level and reads the
 * kept volumes: asked for without them, the call is RSLF_ERR_INVALID_ARG and says so.  The index rules that run off the end
 * in the reference (rslf_render_centre_index, rslf_render_scaled_row) are RSLF_ERR_INVALID_ARG before anything is queued.
 *
 * get_coloured_depth_maps (rslf_fine_to_coarse.hpp:325-378): the fused map of every view through the converter fitted on
 * the fused plane rslf_render_centre_index(S); RSLF_RENDER_AFFINE, black outside the fused validity, shadow cut against
 * level 0's volume.  out: [S][V][U][3]. */
int rslf_f2c_run_render_depth_maps(const rslf_f2c_run* run, rslf_ctx* ctx, int saturate, const uint8_t* lut_bgr, uint8_t* d_bgr_out);
int rslf_f2c_run_render_depth_maps_host(const rslf_f2c_run* run, rslf_ctx* ctx, int saturate, const uint8_t* lut_bgr, uint8_t* h_bgr_out);
/* get_coloured_depth_pyr (:491-519): view s (-1: the centre index) of every level through the converter fitted on level
 * 0's plane before any masking; black outside each level's validity; no shadow cut.  out[l]: [V_l][U_l][3], one pointer
 * per level. */
int rslf_f2c_run_render_depth_pyr(const rslf_f2c_run* run, rslf_ctx* ctx, int s, int saturate, const uint8_t* lut_bgr,
                                  uint8_t* const* d_bgr_out);
int rslf_f2c_run_render_depth_pyr_host(const rslf_f2c_run* run, rslf_ctx* ctx, int s, int saturate, const uint8_t* lut_bgr,
                                       uint8_t* const* h_bgr_out);
/* get_coloured_epi_pyr (:432-488): the S x U_l slice of every level at scanline rslf_render_scaled_row(v, V_l, V_0) (v = -1:
 * the centre index of V_0); invalid pixels count as 0 in the fit (level 0 with its validity) and in the render
 * (RSLF_MASK_ZERO_VALUE); shadow cut against the level's own volume.  out[l]: [S][U_l][3]. */
int rslf_f2c_run_render_epi_pyr(const rslf_f2c_run* run, rslf_ctx* ctx, int v, int saturate, const uint8_t* lut_bgr,
                                uint8_t* const* d_bgr_out);
int rslf_f2c_run_render_epi_pyr_host(const rslf_f2c_run* run, rslf_ctx* ctx, int v, int saturate, const uint8_t* lut_bgr,
                                     uint8_t* const* h_bgr_out);

/* ---- a kept run's peaks per level and validity by uniqueness (K11) ---------- */
/* Two options of a kept run, both off by default, neither in the reference, one device only.
 *
 * peaks = 1: every level's sweep runs in the peaks mode as well (rslf_sweep_peaks above, through the one level loop), and the
 * run keeps four more planes [S][V_p][U_p] per level -- idx, score, runner_idx, runner_score, with the meaning they have
 * there; -1 / 0 where no visit scanned or painted a pixel.  With subgrid = 1 both modes run; `disp` stays in the depth plane.
 * The run also keeps the FUSED peaks at the finest size: four planes [S][V_0][U_0] and a uint8 plane fused_level.  For
 * every pixel of the fused map, fused_level is the level that decided it and the fused peaks are the peaks of the pixel of
 * that level it was taken from.  "Decided" follows the fusion's own mask chain (the INTER_NEAREST upscaling of the running
 * mask, rslf_f2c_fuse): at level p and pixel (y, x), a non-zero validity byte makes that pixel the origin; else the walk goes
 * on at level p + 1, pixel (min(floor(y * (1 / (V_p / V_{p+1}))), V_{p+1} - 1), min(floor(x * (1 / (U_p / U_{p+1}))),
 * U_{p+1} - 1)), scale and product in double.  No valid pixel on the walk: fused_level = 255, idx = runner_idx = -1, the
 * scores 0 -- and the fused validity is 0 there: it is the same chain.  NOTE: the fused DISPARITY of a pixel decided by a
 * coarser level is a bilinear blend of that level's running map followed by the 3 x 3 median; the fused peaks describe the
 * NEAREST pixel of the deciding level, not that blend.  A level accepted whole (accept_all_last_scale) is valid where it
 * has no peaks: such pixels hold -1 / 0 under that level's number.
 *
 * uniqueness_ratio = r in (0, 1] (0: off; needs peaks = 1): after a level's sweep and its validity rule (either
 * RSLF_F2C_VALID_*, any line mode), a pixel becomes invalid if
 *     idx >= 0 && runner_idx >= 0 && runner_score > r * score        (the product one binary32 multiply)
 * and keeps what the rule gave otherwise; the level accept_all_last_scale accepts whole is not touched.  The plane then
 * tightens the next level's ranges and feeds the fusion as ever: an ambiguous pixel of a fine level is decided by a coarser
 * one.  With both options off the entry queues the launches and writes the bits of rslf_f2c_run_host_sub.
 * RSLF_ERR_INVALID_ARG, before anything is queued, with the argument named in rslf_last_error(): peaks outside 0 / 1; a
 * uniqueness_ratio below 0, above 1 or NaN; a ratio without peaks; with peaks, dim_d above 2^24 (rslf_sweep_peaks' limit). */
int rslf_f2c_run_host_pk(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C, size_t row_stride_bytes,
                         float d_min, float d_max, int dim_d, float epi_scale_factor, const rslf_params* p, int max_pyr_depth,
                         int accept_all_last_scale, int line_mode, int validity_rule, int keep_volumes, rslf_f2c_run** run,
                         rslf_stats* stats, int subgrid, int peaks, float uniqueness_ratio);
/* The options read back from a run: 0 for NULL and for a run made without them (rslf_f2c_run_desc keeps its size). */
int rslf_f2c_run_peaks(const rslf_f2c_run* run);
float rslf_f2c_run_uniqueness(const rslf_f2c_run* run);
/* ... and with a last argument propagation_ratio (0: rslf_f2c_run_host_pk, launch for launch): every level's sweep is gated
 * by it (rslf_sweep_propagation_ratio above).  Independent of uniqueness_ratio -- the gate acts inside a level's sweep, the
 * uniqueness on the level's validity after it -- and both may be set.  Needs peaks = 1; a ratio below 0, above 1 or NaN, or
 * one without peaks, is RSLF_ERR_INVALID_ARG before anything is queued.  The run remembers the ratio and, per level, the
 * sources its sweep withheld (0 on every level without the ratio; RSLF_ERR_INVALID_ARG for a level the run does not have). */
int rslf_f2c_run_host_pr(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C, size_t row_stride_bytes,
                         float d_min, float d_max, int dim_d, float epi_scale_factor, const rslf_params* p, int max_pyr_depth,
                         int accept_all_last_scale, int line_mode, int validity_rule, int keep_volumes, rslf_f2c_run** run,
                         rslf_stats* stats, int subgrid, int peaks, float uniqueness_ratio, float propagation_ratio);
float rslf_f2c_run_propagation_ratio(const rslf_f2c_run* run);
int rslf_f2c_run_withheld(const rslf_f2c_run* run, int level, unsigned long long* n);
/* More planes for rslf_f2c_run_copy, reported as bits of planes_held like the others (a run without peaks keeps the bits it
 * had).  PK_*: int32 / float32 [S][V_l][U_l] of any level.  FUSED_PK_* and FUSED_LEVEL (uint8): the finest size, asked for
 * with level 0.  Asked of a run that holds none: RSLF_ERR_INVALID_ARG, `which` named. */
#define RSLF_F2C_PLANE_PK_IDX                 7
#define RSLF_F2C_PLANE_PK_SCORE               8
#define RSLF_F2C_PLANE_PK_RUNNER_IDX          9
#define RSLF_F2C_PLANE_PK_RUNNER_SCORE       10
#define RSLF_F2C_PLANE_FUSED_PK_IDX          11
#define RSLF_F2C_PLANE_FUSED_PK_SCORE        12
#define RSLF_F2C_PLANE_FUSED_PK_RUNNER_IDX   13
#define RSLF_F2C_PLANE_FUSED_PK_RUNNER_SCORE 14
#define RSLF_F2C_PLANE_FUSED_LEVEL           15
/* The two steps as device-pointer primitives, beside rslf_f2c_tighten_bounds and rslf_f2c_fuse: enqueued on the context's
 * stream, not awaited.
 * rslf_f2c_unique_mask: the predicate above in place on n validity bytes; d_pk: idx, score, runner_idx, runner_score of n
 * entries each (disp is ignored); ratio in (0, 1].  Bytes that are 0 stay 0 and their peaks are not read.
 * rslf_f2c_fuse_peaks: the walk above over a pyramid of P levels (1 .. RSLF_F2C_MAX_LEVELS), finest first, in one launch:
 * d_valid[p] and the four planes of d_pk[p] are [S][Vp[p]][Up[p]] (all required; disp ignored); d_out_svu's four planes and
 * d_out_level_svu are [S][Vp[0]][Up[0]], each nullable, not all five.  Any level sizes >= 1 are safe: every index of the
 * walk is clamped into its plane. */
int rslf_f2c_unique_mask(rslf_ctx* ctx, uint8_t* d_valid, const rslf_peaks* d_pk, float ratio, size_t n);
int rslf_f2c_fuse_peaks(rslf_ctx* ctx, const uint8_t* const* d_valid, const rslf_peaks* d_pk, const int* Vp, const int* Up,
                        int P, int S, const rslf_peaks* d_out_svu, uint8_t* d_out_level_svu);

/* ---- cross-view consistency of a sweep's disparity planes (K12) -------- */
/* Not in the reference, whose classes judge a pixel inside its own view (C_e, C_d, C_l): do the views of a finished sweep
 * agree with one another?  A pixel (s, v, u) of disparity d lies, in view t, at column u + (int)roundf(d * (s - t) * slope) of
 * the same scanline -- the propagation's column rule with the pixel's own view for s_hat, both products single and unfused.
 * ok(s, v, u): d_valid_svu is NULL or non-zero there and the disparity is finite.  For an ok pixel and every view t != s in
 * ascending order (radius > 0: only |t - s| <= radius; radius <= 0: every view):
 *   out of field   !(|offset| < 1e9f) -- a NaN included; nothing is converted to int then -- or a column outside [0, U)
 *   seen           the views in field
 *   agree          ... whose pixel there is ok and within tol of d (|d_t - d| <= tol); its disparity joins a running sum
 *   above          ... whose pixel is ok and d_t - d > tol
 *   below          ... whose pixel is ok otherwise
 *   fused          (d + the agreeing disparities, added in ascending t) / (float)(1 + agree): the same bits wherever computed
 *   valid_out      255 where agree >= min_agree, else 0
 * A pixel that is not ok has four counts of 0, fused 0.0f and valid_out 0, and is never agree / above / below for another
 * (the view that shows it still counts as seen).  `above` and `below` stay apart because their meaning depends on the
 * field's sign convention: with disparities that grow towards the camera, a neighbour above is a legitimate occluder and one
 * below a free-space violation; the caller decides.  The rule is stated once, in csrc/k12_consistency_rule.hpp.
 * Planes are [S][V][U]; every output is nullable, not all six; only the planes asked for are written.  No output plane may be
 * an input plane -- d_valid_out_svu may NOT alias d_valid_svu: a thread reads the other views' rows while they are written --
 * and equal pointers are RSLF_ERR_INVALID_ARG, as are a NULL depth plane, S, V or U below 1, a tol that is negative or not
 * finite, and a negative min_agree.  RSLF_ERR_UNSUPPORTED: U above 2^30, or more 256-column segments (8 * ceil(V / 8) * S *
 * ceil(U / 256)) than one launch's grid holds.  One launch, enqueued on the context's stream, not awaited; no scratch. */
typedef struct rslf_view_counts {
    int32_t* seen;     /* [S][V][U], each nullable */
    int32_t* agree;
    int32_t* above;
    int32_t* below;
} rslf_view_counts;
int rslf_view_consistency(rslf_ctx* ctx, const float* d_depth_svu, const uint8_t* d_valid_svu, int S, int V, int U, float slope,
                          float tol, int radius, int min_agree, const rslf_view_counts* d_out, float* d_fused_svu,
                          uint8_t* d_valid_out_svu);
/* The same with every plane on the HOST (d_out -> h_out: host planes): uploads through the context's grow-only staging,
 * runs the launch, downloads the planes asked for and waits.  Refused while a sweep is open on the context. */
int rslf_view_consistency_host(rslf_ctx* ctx, const float* h_depth_svu, const uint8_t* h_valid_svu, int S, int V, int U, float slope,
                               float tol, int radius, int min_agree, const rslf_view_counts* h_out, float* h_fused_svu,
                               uint8_t* h_valid_out_svu);
/* The same on a kept fine-to-coarse run's planes, read in place: RSLF_F2C_PLANE_DEPTH / _VALID of `level`, or -- with
 * fused_result != 0, which needs level 0 -- RSLF_F2C_PLANE_FUSED_MAP / _FUSED_VALID.  The slope is the factor the level's sweep
 * propagated with (U_level / U_0, which the run keeps; 1 for the fused planes).  Outputs: device planes [S][V_level][U_level].
 * ctx: any context of the run's device; enqueued on its stream, not awaited. */
int rslf_f2c_run_consistency(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, float tol, int radius, int min_agree,
                             const rslf_view_counts* d_out, float* d_fused_svu, uint8_t* d_valid_out_svu);
/* ... and with the result planes on the HOST (what rslfx::FineToCoarse holds): staged through the context's grow-only
 * scratch, copied out, awaited.  Refused while a sweep is open on the context. */
int rslf_f2c_run_consistency_host(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, float tol, int radius,
                                  int min_agree, const rslf_view_counts* h_out, float* h_fused_svu, uint8_t* h_valid_out_svu);

/* ---- a kept run's validity by cross-view consistency (K13) -------------- */
/* A third option of a kept run, off by default, not in the reference, one device only.  The validity rule, the uniqueness
 * ratio and the sweep gate all judge a pixel inside its own view; this asks the other views, with the check above, while the
 * pyramid is built.  With consistency_min_agree = m >= 1, after a level's sweep, its validity rule and -- if set -- its
 * uniqueness ratio, a pixel that is still valid becomes invalid unless
 *     consistency_gate(seen, agree, m)  :=  agree >= min(seen, m)
 * with seen and agree as rslf_view_consistency counts them on the level's disparities, that validity (so a pixel the rule or
 * the ratio made invalid neither votes nor is voted on), the level's slope factor, consistency_tol and consistency_radius.
 * At least m of the views that can see the pixel agree with it; where fewer than m can see it, all of them do; a pixel no view
 * can see (seen = 0) is kept -- unlike valid_out above (agree >= min_agree), the rule drops no pixel for lying where its EPI
 * line leaves the field, and no outer view for the radius.  The plane then tightens the next level's ranges and feeds the
 * fusion as ever: a contradicted pixel of a fine level is decided by a coarser one.  The level accept_all_last_scale accepts
 * whole is not touched.  Order within a level: sweep, validity rule, uniqueness, this gate, the next level's ranges.
 * rslf_f2c_run_host_cs is rslf_f2c_run_host_pr plus the three trailing arguments; consistency_min_agree = 0 is that entry,
 * launch for launch and bit for bit (tol and radius are then not looked at).  It needs no peaks and combines with subgrid,
 * peaks, both ratios, any line mode and either validity rule.  RSLF_ERR_INVALID_ARG, before anything is queued, the argument
 * named in rslf_last_error(): a negative consistency_min_agree; with the gate on, a consistency_tol that is negative or not
 * finite, or a sweep left open on the context.  RSLF_ERR_UNSUPPORTED, before anything is queued: rslf_view_consistency's grid limits at the finest level. */
int rslf_f2c_run_host_cs(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C, size_t row_stride_bytes,
                         float d_min, float d_max, int dim_d, float epi_scale_factor, const rslf_params* p, int max_pyr_depth,
                         int accept_all_last_scale, int line_mode, int validity_rule, int keep_volumes, rslf_f2c_run** run,
                         rslf_stats* stats, int subgrid, int peaks, float uniqueness_ratio, float propagation_ratio,
                         float consistency_tol, int consistency_radius, int consistency_min_agree);
/* The pyramid with derivative channels (K17, above): derivative_weight > 0 on a one-channel field (C == 1) runs the raw form
 * once on the finest level's upload and goes on with C = 3 -- every level's downsample, scale, sweep, bound tightening and
 * the fusion run as they do for a three-channel field, bit for bit as the same call on the field (x, fu, fv); a kept run
 * describes itself with C = 3.  0: off, the narrower entry's call.  The two entries are the fullest of their families plus
 * the weight.  RSLF_ERR_INVALID_ARG: a negative or non-finite derivative_weight; RSLF_ERR_UNSUPPORTED: C == 3 with a weight. */
int rslf_fine_to_coarse_run_host_dv(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C,
                                    size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                    const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                    float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats,
                                    int line_mode, const rslf_f2c_levels_out* levels_out, int subgrid, float derivative_weight);
int rslf_f2c_run_host_dv(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C, size_t row_stride_bytes,
                         float d_min, float d_max, int dim_d, float epi_scale_factor, const rslf_params* p, int max_pyr_depth,
                         int accept_all_last_scale, int line_mode, int validity_rule, int keep_volumes, rslf_f2c_run** run,
                         rslf_stats* stats, int subgrid, int peaks, float uniqueness_ratio, float propagation_ratio,
                         float consistency_tol, int consistency_radius, int consistency_min_agree, float derivative_weight);
/* The level dilation (K18; not in the reference): level_dilation = f in 2..8 runs every level's SWEEP on the level's packed
 * volume dilated along u (rslf_volume_dilate_u, kind dilation_kind, the clamp range the packed volume's), U' = f (U_l - 1) + 1
 * wide, with the level's ranges by rslf_planes_dilate_ranges_u and slope_factor = (float)(U_l / U_0) * (float)f, one binary32
 * product.  The dilation never enters the level chain: the raw levels are uploaded, given derivative channels, normalised
 * and downsampled as ever.  The level's planes -- depth, C_e, C_d and the four peak planes -- are the columns u * f of the
 * sweep's, brought back in one launch before anything reads them, so the validity rules, the uniqueness ratio, the
 * consistency gate, the bound tightening, the fusion, the fused peaks, levels_out and a kept run's planes, volumes
 * (undilated) and getters all work on the level's own grid at slope U_l / U_0.  stats.pixels_scanned and a level's withheld
 * count what the sweeps did, in the dilated frame.  level_dilation = 1 is the narrower entry, launch for launch and bit
 * for bit (the kind is still checked).  The two entries are the fullest of their families plus the two arguments.
 * RSLF_ERR_INVALID_ARG, before a device is touched: level_dilation outside 1..8, an unknown dilation_kind;
 * RSLF_ERR_UNSUPPORTED: level_dilation > 1 together with a line-confidence mode (K7 takes no slope factor). */
int rslf_fine_to_coarse_run_host_dl(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C,
                                    size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                    const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                    float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats,
                                    int line_mode, const rslf_f2c_levels_out* levels_out, int subgrid, float derivative_weight,
                                    int level_dilation, int dilation_kind);
int rslf_f2c_run_host_dl(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C, size_t row_stride_bytes,
                         float d_min, float d_max, int dim_d, float epi_scale_factor, const rslf_params* p, int max_pyr_depth,
                         int accept_all_last_scale, int line_mode, int validity_rule, int keep_volumes, rslf_f2c_run** run,
                         rslf_stats* stats, int subgrid, int peaks, float uniqueness_ratio, float propagation_ratio,
                         float consistency_tol, int consistency_radius, int consistency_min_agree, float derivative_weight,
                         int level_dilation, int dilation_kind);
/* The two read back (each pointer nullable): 1 and RSLF_DILATE_CUBIC for NULL and for a run made without the dilation. */
int rslf_f2c_run_level_dilation(const rslf_f2c_run* run, int* factor, int* kind);
/* The pyramid on a field equalised per view (K19, above): equalize_mode = RSLF_EQUALIZE_GAIN or _AFFINE runs
 * rslf_equalize_views_dense once, in place, on the finest level's upload -- hi the element type's 255 or 65535, for float
 * elements the upload's maximum -- before the derivative channels, so the features are derivatives of the equalised
 * intensity, and then goes on unchanged: bit for bit the same call on the equalised field.  equalize_ref_view: the view whose
 * statistics are the target, -1 for the views' mean; equalize_joint: one pair for the three channels (C == 3);
 * equalize_max_gain: the clamp of the gain.  equalize_mode = 0: off, the narrower entry's call, launch for launch and bit for
 * bit; no launch, no allocation, and the three other arguments are not looked at.  The two entries are the fullest of their
 * families plus the four arguments.  RSLF_ERR_INVALID_ARG, before a device is touched: an unknown mode, equalize_ref_view
 * outside [-1, S), an equalize_max_gain that is not finite or < 1, equalize_joint with C == 1; RSLF_ERR_UNSUPPORTED, before a
 * device is touched too: V * U beyond 2^31 - 1 (with equalize_joint: beyond 1431699457); after the upload: a float field whose maximum is not finite and > 0.  The multi-device loop refuses the option by name. */
int rslf_fine_to_coarse_run_host_eq(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C,
                                    size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                    const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                    float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats,
                                    int line_mode, const rslf_f2c_levels_out* levels_out, int subgrid, float derivative_weight,
                                    int level_dilation, int dilation_kind, int equalize_mode, int equalize_ref_view,
                                    int equalize_joint, float equalize_max_gain);
int rslf_f2c_run_host_eq(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C, size_t row_stride_bytes,
                         float d_min, float d_max, int dim_d, float epi_scale_factor, const rslf_params* p, int max_pyr_depth,
                         int accept_all_last_scale, int line_mode, int validity_rule, int keep_volumes, rslf_f2c_run** run,
                         rslf_stats* stats, int subgrid, int peaks, float uniqueness_ratio, float propagation_ratio,
                         float consistency_tol, int consistency_radius, int consistency_min_agree, float derivative_weight,
                         int level_dilation, int dilation_kind, int equalize_mode, int equalize_ref_view, int equalize_joint,
                         float equalize_max_gain);
/* The settings read back (each pointer nullable): mode 0 and view 0 for NULL and for a run made without the equalisation;
 * h_a_b [S][C][2], C the field's own channel count, receives the coefficients the run applied and is left untouched by a run
 * made without it. */
int rslf_f2c_run_equalize(const rslf_f2c_run* run, int* mode, int* ref_view, float* h_a_b);
/* C of that h_a_b: the channels of the field the run was made from (1 for a run with derivative channels, which describes
 * itself with C = 3); 0 for NULL and for a run made without the equalisation.  Returns the count, not a status. */
int rslf_f2c_run_view_gains_channels(const rslf_f2c_run* run);
/* The options read back (each pointer nullable): zeros for NULL and for a run made without the gate. */
int rslf_f2c_run_consistency_gate(const rslf_f2c_run* run, float* tol, int* radius, int* min_agree);
/* The pixels the gate made invalid on `level`: 0 for a level accepted whole and for every level of a run made without the
 * gate; RSLF_ERR_INVALID_ARG for a level the run does not have. */
int rslf_f2c_run_inconsistent(const rslf_f2c_run* run, int level, unsigned long long* n);
/* Two more planes for rslf_f2c_run_copy, int32 [S][V_l][U_l] of any gated level, reported as bits 16 and 17 of planes_held (a
 * run without the gate keeps the planes_held and device_bytes it had): the gate's OWN counts at gate time, which explain a
 * drop.  rslf_f2c_run_consistency run afterwards reads the gated validity and counts differently.  Asked of a run or a level
 * that holds none (the level accepted whole): RSLF_ERR_INVALID_ARG, `which` named. */
#define RSLF_F2C_PLANE_CS_AGREE 16
#define RSLF_F2C_PLANE_CS_SEEN  17
/* The gate as a device-pointer primitive, beside rslf_f2c_unique_mask: one launch, enqueued on the context's stream, not
 * awaited; no scratch.  d_valid_svu is required (it is what the gate gates); d_valid_out_svu [S][V][U] receives the input byte
 * where the pixel is kept -- a pixel that is not ok (byte 0, or a non-finite disparity) is kept as it is -- and 0 where it is
 * dropped, and may NOT be d_valid_svu: a thread reads the other views' rows while they are written.  d_agree_svu / d_seen_svu
 * (nullable): the two counts, 0 where the pixel is not ok.  d_dropped (nullable): a device counter the launch ADDS the number
 * of pixels it made invalid to (one 64-bit atomic per 256-column segment that dropped any); the caller zeroes it.
 * Refusals: rslf_view_consistency's, with min_agree >= 1 required. */
int rslf_f2c_consistency_mask(rslf_ctx* ctx, const float* d_depth_svu, const uint8_t* d_valid_svu, int S, int V, int U, float slope,
                              float tol, int radius, int min_agree, uint8_t* d_valid_out_svu, int32_t* d_agree_svu,
                              int32_t* d_seen_svu, unsigned long long* d_dropped);

/* ---- the view warp: any view position from a sweep's planes (K14) -------- */
/* Not in the reference.  The check above looks along a pixel's own EPI line; this asks the opposite: what does a view at
 * position t look like, given what the views hold?  A scatter with an occlusion order -- render a view nobody took, fill a view
 * from the others, or (with a view excluded from its own prediction) measure how well the disparities explain the light field.
 * t is a float, finite, |t| <= 65536; it need not be integral and need not lie inside [0, S - 1].  A source pixel (s, v, u) of
 * disparity d is a CANDIDATE for column x of scanline v of target t when it is ok (as above: d_valid_svu NULL or non-zero there,
 * d finite), s != exclude, radius <= 0 or fabsf((float)s - t) <= (float)radius, and
 *     x = u + (int)roundf(fl(fl(d * fl((float)s - t)) * slope))
 * is in [0, U) with the offset below 1e9f in magnitude (a NaN is never converted) -- for an integral t the column rule above,
 * bit for bit.  Among the candidates of (v, x) the WINNER has the greatest z = nearer >= 0 ? d : -d (-0.0f and +0.0f are equal;
 * nearer = +1: larger disparities are nearer, the reference's occlusion map and rslf_render_epi_lines' order; -1: the opposite
 * convention); among equal z the smaller fabsf((float)s - t); among equal distances the smaller s.  The order is total, so the
 * result does not depend on the order the sources are visited in.  The rule is stated once, in csrc/k14_warp_rule.hpp.
 * Outputs per target k of the T targets, each nullable, not all nine; only the planes asked for are written:
 *   hit       u8  [T][V][U]     255 where a candidate arrived, else 0
 *   depth     f32 [T][V][U]     the winner's stored disparity, its own bits; 0 where none
 *   src_view  i32 [T][V][U]     the winner's s; -1 where none
 *   src_col   i32 [T][V][U]     the winner's u; -1 where none
 *   count     i32 [T][V][U]     the candidates that arrived, winners or not
 *   colour    f32 [T][V][U][C]  the volume's radiance at (v, src_view, src_col, :), as it holds it (normalised); 0 where none
 *   err       f32 [T][V][U]     the leave-one-out residual against the slab's own row (v, t): acc = 0; for c ascending:
 *                               acc = acc + fabsf(colour[c] - L[x][c]); acc / (float)C; 0 where none
 *   row_err   f64 [T][V]        the sum of err over a row's hit pixels, in double, in an order left open
 *   row_hits  i32 [T][V]        their number
 * colour, err and row_err need `volume` (else nullable), of the planes' V, S, U; err and row_err also need every target to be a
 * view: integral and in [0, S).  targets [T] and exclude [T] (nullable: nobody; an entry of -1: nobody) are HOST arrays, read
 * before the return.  RSLF_ERR_INVALID_ARG, before anything is queued, the argument named in rslf_last_error(): a NULL depth
 * plane or targets, S, V or U below 1, T below 1, nearer == 0, no output, an output plane that is an input plane, a volume
 * missing or of another shape, a target that is not finite or beyond 65536 (for err: not a view).  RSLF_ERR_UNSUPPORTED: U
 * above 8192 (the z-buffer of a row, one 64-bit key per column in LDS), S above 65536, or T * 8 * ceil(V / 8) not below 2^31.
 * One launch per 256 targets, enqueued on the context's stream, not awaited; no scratch. */
typedef struct rslf_view_warp_out {
    uint8_t* hit;
    float* depth;
    int32_t* src_view;
    int32_t* src_col;
    int32_t* count;
    float* colour;
    float* err;
    double* row_err;
    int32_t* row_hits;
} rslf_view_warp_out;
int rslf_view_warp(rslf_ctx* ctx, const float* d_depth_svu, const uint8_t* d_valid_svu, int S, int V, int U, float slope,
                   const rslf_volume* volume, const float* targets, const int* exclude, int T, int radius, int nearer,
                   const rslf_view_warp_out* d_out);
/* The same with the planes on the HOST (the volume stays a device object): uploads through the context's grow-only staging,
 * runs the launches, downloads the planes asked for and waits.  Refused while a sweep is open on the context. */
int rslf_view_warp_host(rslf_ctx* ctx, const float* h_depth_svu, const uint8_t* h_valid_svu, int S, int V, int U, float slope,
                        const rslf_volume* volume, const float* targets, const int* exclude, int T, int radius, int nearer,
                        const rslf_view_warp_out* h_out);
/* The same on a kept fine-to-coarse run's planes, read in place, as rslf_f2c_run_consistency reads them: a level's depth and
 * validity, or with fused_result != 0 (level 0) the fused pair; the slope the level ran with; the level's kept volume.  A run
 * made without keep_volumes refuses colour, err and row_err by name.  ctx: any context of the run's device. */
int rslf_f2c_run_view_warp(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, const float* targets, const int* exclude,
                           int T, int radius, int nearer, const rslf_view_warp_out* d_out);
/* ... and with the result planes on the HOST: staged, copied out, awaited.  Refused while a sweep is open on the context. */
int rslf_f2c_run_view_warp_host(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, const float* targets,
                                const int* exclude, int T, int radius, int nearer, const rslf_view_warp_out* h_out);

/* ---- the novel view: the warp's holes filled, the views that see a point blended (K15) -------- */
/* Not in the reference.  The warp above stops at one source pixel per target pixel, or nothing.  This is the second half of
 * depth-image-based rendering: a finished image of view position t.  Per target and scanline, three stages; the rule is
 * stated once, in csrc/k15_novel_rule.hpp.
 *   A  z-buffer   the warp's rule unchanged (exclude, params->radius, params->nearer): per column a hit and the winner's
 *                 stored disparity, its own bits.
 *   B  fill       a RUN is a maximal stretch of columns without a hit, n columns long, with the column before it as its
 *                 left bound (none at the row's start) and the column after it as its right bound (none at the row's end).
 *                 It stays a hole with no bound at all, or when max_gap > 0 && n > max_gap.  Otherwise every column of it
 *                 takes the disparity of one bound: the only one, or of two the FARTHER (the smaller z; a disocclusion
 *                 belongs to the background), the left one on equal z.
 *   C  gather     for a pixel x that is not a hole, of disparity d, the views are walked by (distance to t, s); the walk
 *                 stops at the first view outside the radius and skips `exclude`.  For view s
 *                     off = fl(fl(d * fl((float)s - t)) * slope)     out of field unless fabsf(off) < 1e9f
 *                     p = (float)x - off,  ur = (int)roundf(p)       out of field unless ur in [0, U)
 *                 and the view AGREES when depth[s][v][ur] is ok and fabsf(depth[s][v][ur] - d) <= tol.  Its sample is
 *                     i0 = floorf(p), i1 = ceilf(p), w = p - (float)i0, both taps clamped into [0, U - 1]
 *                     sample[c] = (1 - w) * E[i0][c] + w * E[i1][c]    (two products, one sum, no FMA)
 *                 An agreeing view joins the blend with weight g = 1.0f / (1.0f + fabsf((float)s - t)), in walk order:
 *                 acc[c] = acc[c] + g * sample[c], wsum = wsum + g; the walk ends after `sources` agreeing views.
 * Outputs per target k of the T targets, each nullable, not all seven; only the planes asked for are written:
 *   colour   f32 [T][V][U][C]  acc[c] / wsum where n_src > 0; where nobody agreed the sample of the FIRST view of the walk
 *                              that was in field, unverified; 0 if none was, and 0 at a hole
 *   depth    f32 [T][V][U]     the winner's stored disparity at hits, the bound's bits at filled pixels, 0 at holes
 *   fill     u8  [T][V][U]     0 hole, 1 hit, 2 filled from the left bound, 3 filled from the right bound
 *   n_src    i32 [T][V][U]     the views blended
 *   err      f32 [T][V][U]     the residual of colour against the slab's own row (v, t), as rslf_view_warp's, wherever a
 *                              colour was taken from a view; else 0
 *   row_err  f64 [T][V]        the sum of err over a row's pixels with n_src > 0, in double, in an order left open
 *   row_cov  i32 [T][V]        their number
 * colour, err and row_err need `volume`; depth, fill, n_src and row_cov do not.  err and row_err need every target to be a
 * view.  RSLF_ERR_INVALID_ARG as rslf_view_warp, and: params NULL, sources < 1, tol negative or a NaN (+inf accepts every ok
 * pixel), nearer == 0, no output, an output plane that is an input plane.  RSLF_ERR_UNSUPPORTED as rslf_view_warp (U above
 * 8192, S above 65536, the grid).  One launch per 256 targets, enqueued on the context's stream, not awaited; no scratch. */
typedef struct rslf_novel_view_params {
    int radius, nearer, max_gap, sources;
    float tol;
} rslf_novel_view_params;
typedef struct rslf_novel_view_out {
    float* colour;
    float* depth;
    uint8_t* fill;
    int32_t* n_src;
    float* err;
    double* row_err;
    int32_t* row_cov;
} rslf_novel_view_out;
int rslf_novel_view(rslf_ctx* ctx, const float* d_depth_svu, const uint8_t* d_valid_svu, int S, int V, int U, float slope,
                    const rslf_volume* volume, const float* targets, const int* exclude, int T, const rslf_novel_view_params* params,
                    const rslf_novel_view_out* d_out);
/* The same with the planes on the HOST (the volume stays a device object): staged through the context's buffers, awaited.
 * Refused while a sweep is open on the context. */
int rslf_novel_view_host(rslf_ctx* ctx, const float* h_depth_svu, const uint8_t* h_valid_svu, int S, int V, int U, float slope,
                         const rslf_volume* volume, const float* targets, const int* exclude, int T, const rslf_novel_view_params* params,
                         const rslf_novel_view_out* h_out);
/* The same on a kept fine-to-coarse run's planes, read in place, as rslf_f2c_run_view_warp reads them.  A run made without
 * keep_volumes refuses colour, err and row_err by name. */
int rslf_f2c_run_novel_view(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, const float* targets, const int* exclude,
                            int T, const rslf_novel_view_params* params, const rslf_novel_view_out* d_out);
/* ... and with the result planes on the HOST: staged, copied out, awaited.  Refused while a sweep is open on the context. */
int rslf_f2c_run_novel_view_host(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, const float* targets,
                                 const int* exclude, int T, const rslf_novel_view_params* params, const rslf_novel_view_out* h_out);

/* Depth2DComputer<T>'s constructor + run() + getters (rslf_depth_computation.hpp:651-805) over the context's devices,
 * host EPIs in, host [S][V][U] planes out.  The 2-D sweep is cut into one block of scanlines per device; every visit
 * exchanges the neighbours' boundary rows (median reach) of the visited view's raw disparities and edge mask by peer
 * copy between the scan and the median -- the one exchange step of the path.  One host thread queues the work of all
 * devices; events keep the order.  Planes may be NULL (not wanted).  Bit-identical to rslf_depth2d_run on one volume. */
int rslf_multi_depth2d_run_f32(rslf_multi* m, const float* const* h_epis, size_t row_stride_bytes, int V, int S, int U, int C,
                               float epi_scale_factor, float dmin, float dmax, int dim_d, const rslf_params* p,
                               float* h_Ce_svu, uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu,
                               float* h_rbar_svu, uint8_t* h_scan_mask_svu, rslf_stats* stats, float* scale_used);
int rslf_multi_depth2d_run_u8(rslf_multi* m, const uint8_t* const* h_epis, size_t row_stride_bytes, int V, int S, int U, int C,
                              float dmin, float dmax, int dim_d, const rslf_params* p, float* h_Ce_svu,
                              uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu, float* h_rbar_svu,
                              uint8_t* h_scan_mask_svu, rslf_stats* stats);
/* CV_16U EPIs: arguments as rslf_multi_depth2d_run_f32, bit-identical to it on the same values. */
int rslf_multi_depth2d_run_u16(rslf_multi* m, const uint16_t* const* h_epis, size_t row_stride_bytes, int V, int S, int U, int C,
                               float epi_scale_factor, float dmin, float dmax, int dim_d, const rslf_params* p,
                               float* h_Ce_svu, uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu,
                               float* h_rbar_svu, uint8_t* h_scan_mask_svu, rslf_stats* stats, float* scale_used);

/* FineToCoarse<T>'s constructor + run() + get_results() (rslf_fine_to_coarse.hpp:103-324) over the context's devices:
 * every level's 2-D sweep runs sharded as in rslf_multi_depth2d_run_* (with the level's tightened per-pixel ranges); the
 * pyramid, the bound tightening and the fusion run on the first device, which also holds every level's planes: the
 * other devices fetch their rows from it and return their results to it by peer copies.
 * Arguments and results as rslf_fine_to_coarse_run_host; bit-identical to it. */
int rslf_multi_fine_to_coarse_run_host(rslf_multi* m, const void* const* h_epis, int is_u8, int V, int S, int U, int C,
                                       size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                       const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                       float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats);
int rslf_multi_fine_to_coarse_run_host_u16(rslf_multi* m, const uint16_t* const* h_epis, int V, int S, int U, int C,
                                           size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                           const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                           float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats);

/* ---- rendering: the getters' pictures (K6) ------------------------------- */
/* What the reference's getters do between run() and imshow: scale a plane to 8 bits, map it through a colour table,
 * black out what the masks reject.  cv::applyColorMap lives in OpenCV, not in the reference, so the library knows no
 * colour map by name: every render entry takes `lut_bgr`, a HOST table of 256 x 3 bytes (copied to the device once per
 * call), and level i becomes lut_bgr[3 i .. 3 i + 2].  Pictures are uint8 BGR like the reference's CV_8UC3, dense.
 * Planes, masks and pictures are device pointers (host pointers in the *_host forms); strides are in elements.  A NaN in a plane (cv::sort and minMaxLoc
 * are undefined on one) neither faults nor hangs; what comes back for it is unspecified. */
#define RSLF_FIT_MINMAX    0   /* cv::minMaxLoc, as copy_and_scale_uchar takes them -- src/rslf_plot.cpp:52-53 */
#define RSLF_FIT_QUANTILE  1   /* ImageConverter_uchar::fit(img, true), :70-84: elements floor(0.02 N) and floor(0.98 N) of the
                                  ascending sort, N = rows * cols -- here an exact radix select, no sort */
#define RSLF_FIT_MEANSTD   2   /* fit(img, false), :85-95: min = true min, max = min(mean + 12 std, true max), double sums */
#define RSLF_FIT_GIVEN     3   /* rslf_render_planes_host alone: no fit, plane k goes through h_minmax[k][0 .. 1], which is then an
                                  input -- a level of a pyramid through the converter fitted on another level */
#define RSLF_RENDER_SHIFT  0   /* copy_and_scale_uchar, :41-63: (x - (float)min) * (float)(255.0 / (max - min)) */
#define RSLF_RENDER_AFFINE 1   /* ImageConverter_uchar::copy_and_scale, :100-107: x * alpha + beta, alpha = (float)(255.0 / (max - min)),
                                  beta = (float)(-(double)alpha * min) */
#define RSLF_MASK_BLACK      0 /* the pixel goes black after the look-up where the mask byte is 0
                                  (setTo(0, validity == 0), include/rslf_fine_to_coarse.hpp:356, :514; cv::add under a mask,
                                  include/rslf_depth_computation.hpp:638) */
#define RSLF_MASK_ZERO_VALUE 1 /* the VALUE counts as 0.0f before the level is taken: the pixel gets the colour of level(0), not
                                  black (get_coloured_epi_pyr, include/rslf_fine_to_coarse.hpp:458-459 before :465-466) */
#define RSLF_SLICE_VIEW    0   /* plane k is view s = index + k of the volume, its rows are scanlines v */
#define RSLF_SLICE_EPI     1   /* the plane is scanline v = index, its rows are views s (rslf_render_planes_each and
                                  rslf_render_planes_host: plane k is scanline index + k) */

/* The two numbers a converter holds (ImageConverter_uchar::min / max, include/rslf_plot.hpp:63-64; the min / max of
 * copy_and_scale_uchar) for a plane of rows x cols floats, `row_stride` elements from row to row -- so row v of an
 * [S][V][U] stack is fitted as an S x U plane.  d_valid (nullable, same strides): a pixel whose byte is 0 counts as
 * 0.0f (include/rslf_fine_to_coarse.hpp:458-459).  mode: RSLF_FIT_*.  Integer counts and fixed-order double sums: the
 * same bits on every run. */
int rslf_render_fit(rslf_ctx* ctx, const float* d_plane, int rows, int cols, size_t row_stride, const uint8_t* d_valid, int mode,
                    double* h_min, double* h_max);   /* returns the values: waits */
/* The same for n_planes planes (1 .. 65535) of one stack, plane k starting plane_stride elements after plane k - 1, in
 * launches whose number does not depend on n_planes, one copy to the host and one wait: h_minmax [n_planes][2] gets
 * (min, max) of every plane, bit for bit what rslf_render_fit returns for that plane alone.  Every view of an [S][V][U]
 * stack: n_planes = S, plane_stride = V * U, rows = V, row_stride = U; every EPI slice of it: n_planes = V,
 * plane_stride = U, rows = S, row_stride = V * U.  d_valid (nullable): same strides. */
int rslf_render_fit_many(rslf_ctx* ctx, const float* d_planes, int n_planes, size_t plane_stride, int rows, int cols, size_t row_stride,
                         const uint8_t* d_valid, int mode, double* h_minmax);   /* returns the values: waits */
/* Level -> table -> mask -> shadow cut for n_planes planes in one launch (the loops of get_disparity_map,
 * get_coloured_epi of Depth2DComputer, get_coloured_depth_maps, get_coloured_depth_pyr, get_coloured_epi_pyr --
 * include/rslf_depth_computation.hpp:619-643, :808-891, include/rslf_fine_to_coarse.hpp:325-378, :432-519).
 * Plane k starts plane_stride elements after plane k - 1.  formula: RSLF_RENDER_*, then cvRound (nearest even) and
 * saturate_cast<uchar>.  d_valid (nullable, same strides) acts as mask_mode (RSLF_MASK_*) says.  vol (nullable): the
 * shadow cut, applied last -- a pixel goes black when the norm of the volume's radiance at its (v, s, u) is below
 * shadow_level (include/rslf_fine_to_coarse.hpp:360-372, :466-481); slice_kind / index (RSLF_SLICE_*) say where the
 * planes lie in the volume.  d_bgr_out: [n_planes][rows][cols][3]. */
int rslf_render_planes(rslf_ctx* ctx, const float* d_planes, int n_planes, size_t plane_stride, int rows, int cols, size_t row_stride,
                       double min, double max, int formula, const uint8_t* lut_bgr, const uint8_t* d_valid, int mask_mode,
                       const rslf_volume* vol, int slice_kind, int index, float shadow_level, uint8_t* d_bgr_out);
/* rslf_render_planes with a range per plane: plane k goes through h_minmax[k][0 .. 1] (HOST, [n_planes][2], as
 * rslf_render_fit_many fills it).  With RSLF_SLICE_EPI the batch may hold several planes: plane k is scanline index + k,
 * index + n_planes <= V.  Enqueued, not awaited, like rslf_render_planes. */
int rslf_render_planes_each(rslf_ctx* ctx, const float* d_planes, int n_planes, size_t plane_stride, int rows, int cols, size_t row_stride,
                            const double* h_minmax, int formula, const uint8_t* lut_bgr, const uint8_t* d_valid, int mask_mode,
                            const rslf_volume* vol, int slice_kind, int index, float shadow_level, uint8_t* d_bgr_out);
/* Fit and render with planes, validity and pictures on the HOST (what the classes of rslf_hip.hpp hold): uploads the
 * stack, fits (fit_mode: RSLF_FIT_*; fit_plane = -1: every plane through its own range, by rslf_render_fit_many;
 * fit_plane = k >= 0: every plane through plane k's range, as FineToCoarse::get_coloured_depth_maps does; fit_masked != 0:
 * the fit sees h_valid, as rslf_render_fit's d_valid), renders as rslf_render_planes_each / rslf_render_planes do, downloads
 * and waits.  h_valid: nullable.  vol (nullable) is a device volume of this context.  h_bgr_out: [n_planes][rows][cols][3].
 * h_minmax (nullable): [n_planes][2], the ranges used.  Staging is the context's grow-only scratch: a second call of the
 * same size allocates nothing. */
int rslf_render_planes_host(rslf_ctx* ctx, const float* h_planes, int n_planes, size_t plane_stride, int rows, int cols, size_t row_stride,
                            const uint8_t* h_valid, int fit_mode, int fit_plane, int fit_masked, int formula, const uint8_t* lut_bgr,
                            int mask_mode, const rslf_volume* vol, int slice_kind, int index, float shadow_level, uint8_t* h_bgr_out,
                            double* h_minmax);
/* Depth1DComputer_pile::get_coloured_epi and Depth1DComputer::get_coloured_epi --
 * include/rslf_depth_computation.hpp:568-617, :374-416 -- for scanlines v_first .. v_first + n_rows - 1 of the planes
 * [V][U]: every masked column u draws, in view s, the column u + (int)std::round(depth * (float)(s_hat - s)) (columns
 * > -1, the pile's test) in the colour of its depth, scaled by RSLF_RENDER_SHIFT over the min and max of the scanline's
 * U depths, masked or not (:587).  A target keeps the source with the greatest depth, of equal depths the smallest u:
 * the loop's sequential meaning (under OpenMP the reference's loop races).  Pixels no line reaches stay black; a NaN depth
 * draws nothing.  d_bgr_out: [n_rows][S][U][3]. */
int rslf_render_epi_lines(rslf_ctx* ctx, const float* d_depth_vu, const uint8_t* d_mask_vu, int V, int S, int U, int s_hat, int v_first,
                          int n_rows, const uint8_t* lut_bgr, uint8_t* d_bgr_out);
/* The same with depths, mask and picture on the host: uploads the n_rows scanlines, paints, downloads and waits. */
int rslf_render_epi_lines_host(rslf_ctx* ctx, const float* h_depth_vu, const uint8_t* h_mask_vu, int V, int S, int U, int s_hat, int v_first,
                               int n_rows, const uint8_t* lut_bgr, uint8_t* h_bgr_out);
/* The getters' two index rules, which both run off the end in the reference (it then reads out of bounds); these
 * return RSLF_ERR_INVALID_ARG there and say why.  std::round: halves away from zero.
 * (int)std::round(n / 2.0): the plane FineToCoarse fits on and shows -- include/rslf_fine_to_coarse.hpp:344, :497;
 * n itself for n = 1. */
int rslf_render_centre_index(int n, int* index);
/* (int)std::round(1.0 * v * dim_v / dim_v_orig): the scanline of a pyramid level that get_coloured_epi_pyr shows for
 * scanline v of the finest -- include/rslf_fine_to_coarse.hpp:451; dim_v itself for v = dim_v_orig - 1 where
 * dim_v = dim_v_orig / 2 (the getter's default v, round(dim_v_orig / 2.0), is out of range for dim_v_orig = 1). */
int rslf_render_scaled_row(int v, int dim_v, int dim_v_orig, int* row);

/* ---- measurement ------------------------------------------------------ */
/* Duration in milliseconds of the last scan-kernel launch (K2) of this
 * context, from HIP events recorded on the context's stream around that
 * launch.  Blocks until the launch has finished.  Within a 2-D sweep only
 * the first (dense, centre-view) visit is timed: an event is a packet of
 * its own in the queue, and two per sparse visit cost a tenth of the visit. */
int rslf_last_scan_kernel_ms(rslf_ctx* ctx, float* ms);
/* With rslf_ctx_set_debug(ctx, "time_all", 1): the SUM of the durations of every scan launch sequence queued on this
 * context since the last call (or since the hook was set) and their number; blocks until they have finished, then starts
 * a new sum.  For the roofline of the rows around the path: a 2-D sweep is one dense and S - 1 sparse scan launches, a
 * fine-to-coarse run that per pyramid level (core.hpp:993-1028). */
int rslf_scan_time_total_ms(rslf_ctx* ctx, float* ms, int* launches);
/* What the last scan of this context took from the row-exact table ("scalar_taps"): *attached = 1 if its launch was handed
 * one (0: the kernel has no scalar-tap form, a hook is off, per-pixel ranges, a packed launch), *exact_hypotheses = how many
 * hypotheses of that table are row-exact -- the ones whose interior tiles ran the scalar-tap form.  Waits for the stream. */
int rslf_last_scan_row_exact(rslf_ctx* ctx, int* attached, int* exact_hypotheses);

#ifdef __cplusplus
}
#endif
#endif /* RSLF_HIP_H */
