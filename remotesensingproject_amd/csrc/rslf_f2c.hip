// librslf_hip.so, unit 7 of 9: fine-to-coarse (rslf_fine_to_coarse.hpp:103-324, rslf_fine_to_coarse_core.cpp:14-135) --
// the pyramid (Gaussian blur + halving), the bound tightening, the fusion (K5) and the native level loop, whose one-context
// form is here and whose multi-device form is in rslf_multi_sweep.hip.  C-ABI: include/rslf_hip.h.
#include "rslf_internal.hpp"
#include "rslf_plan_derivative.hpp"
#include "k19_equalize_rule.hpp"
#include "rslf_plan_dilate.hpp"
#include "rslf_plan_f2c_consistency.hpp"
#include "rslf_plan_f2c_peaks.hpp"

#include <algorithm>
#include <cmath>
#include <stdexcept>

#include "k5_f2c.hpp"

using namespace rslf;

// ---- "next" row: fine-to-coarse ------------------------------------------------

extern "C" int rslf_f2c_level_dims(int V, int U, int* V2, int* U2) RSLF_API_TRY
{
    if (!V2 || !U2 || V < 1 || U < 1)
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    plan::f2c_level_dims(V, U, V2, U2);   // cvRound: ties to even
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_downsample_epis_f32(rslf_ctx* ctx, const float* d_in_vsuc, int V, int S, int U, int C, float* d_out_vsuc) RSLF_API_TRY
{
    if (!ctx || !d_in_vsuc || !d_out_vsuc || V < 1 || S < 1 || U < 1 || (C != 1 && C != 3))
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(ctx->device));
    int V2, U2;
    rslf_f2c_level_dims(V, U, &V2, &U2);
    if (V2 < 1 || U2 < 1)
        return fail(RSLF_ERR_INVALID_ARG, "level too small to halve");
    void* tmp_p = nullptr;
    int rc = helper_scratch(ctx, kSharedLevel, (size_t)V * S * U * C * sizeof(float), &tmp_p);
    if (rc)
        return rc;
    hipStream_t st = ctx->stream;
    const long long row_blocks = (long long)V * S * ((U * C + 255) / 256);
    if (row_blocks > (1ll << 31) - 1)
        return fail(RSLF_ERR_UNSUPPORTED, "volume too large for one downsampling launch");
    hipLaunchKernelGGL(k5_gauss_rows, dim3((unsigned)row_blocks), dim3(256), 0, st, d_in_vsuc, (float*)tmp_p, (long long)V * S, U, C);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k5_gauss_cols_halve, dim3((U2 * C + 255) / 256, S, V2), dim3(256), 0, st, (const float*)tmp_p, d_out_vsuc,
                       V, S, U, C, V2, U2);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;   // enqueued on the context's stream like every device entry point
}
RSLF_API_CATCH

extern "C" int rslf_downsample_epis_u8(rslf_ctx* ctx, const float* d_in_vsuc, int V, int S, int U, int C, float* d_out_vsuc) RSLF_API_TRY
{
    if (!ctx || !d_in_vsuc || !d_out_vsuc || V < 1 || S < 1 || U < 1 || (C != 1 && C != 3))
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(ctx->device));
    int V2, U2;
    rslf_f2c_level_dims(V, U, &V2, &U2);
    if (V2 < 1 || U2 < 1)
        return fail(RSLF_ERR_INVALID_ARG, "level too small to halve");
    void* tmp_p = nullptr;
    int rc = helper_scratch(ctx, kSharedLevel, (size_t)V * S * U * C * sizeof(int), &tmp_p);
    if (rc)
        return rc;
    hipStream_t st = ctx->stream;
    const long long row_blocks = (long long)V * S * ((U * C + 255) / 256);
    if (row_blocks > (1ll << 31) - 1)
        return fail(RSLF_ERR_UNSUPPORTED, "volume too large for one downsampling launch");
    hipLaunchKernelGGL(k5_gauss_rows_u8, dim3((unsigned)row_blocks), dim3(256), 0, st, d_in_vsuc, (int*)tmp_p, (long long)V * S, U, C);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k5_gauss_cols_halve_u8, dim3((U2 * C + 255) / 256, S, V2), dim3(256), 0, st, (const int*)tmp_p, d_out_vsuc,
                       V, S, U, C, V2, U2);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_downsample_epis_u16(rslf_ctx* ctx, const float* d_in_vsuc, int V, int S, int U, int C, float* d_out_vsuc) RSLF_API_TRY
{
    if (!ctx || !d_in_vsuc || !d_out_vsuc || V < 1 || S < 1 || U < 1 || (C != 1 && C != 3))
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(ctx->device));
    int V2, U2;
    rslf_f2c_level_dims(V, U, &V2, &U2);
    if (V2 < 1 || U2 < 1)
        return fail(RSLF_ERR_INVALID_ARG, "level too small to halve");
    void* tmp_p = nullptr;
    int rc = helper_scratch(ctx, kSharedLevel, (size_t)V * S * U * C * sizeof(float), &tmp_p);
    if (rc)
        return rc;
    hipStream_t st = ctx->stream;
    const long long row_blocks = (long long)V * S * ((U * C + 255) / 256);
    if (row_blocks > (1ll << 31) - 1)
        return fail(RSLF_ERR_UNSUPPORTED, "volume too large for one downsampling launch");
    hipLaunchKernelGGL(k5_gauss_rows, dim3((unsigned)row_blocks), dim3(256), 0, st, d_in_vsuc, (float*)tmp_p, (long long)V * S, U, C);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k5_gauss_cols_halve_u16, dim3((U2 * C + 255) / 256, S, V2), dim3(256), 0, st, (const float*)tmp_p, d_out_vsuc,
                       V, S, U, C, V2, U2);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_device_max_f32(rslf_ctx* ctx, const float* d_values, size_t n, float* h_max) RSLF_API_TRY
{
    if (!ctx || !d_values || !h_max || n == 0)
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(ctx->device));
    const int blocks = (int)std::min<size_t>((n + 255) / 256, Scratch::kMaxPartials);
    HIP_TRY(hip_err(ctx->scratch.max_partial.reserve(Scratch::kMaxPartials * sizeof(float))));   // 8 KiB of its own
    float* const part_p = ctx->scratch.max_partial.as<float>();
    hipLaunchKernelGGL(k5_max_partial, dim3(blocks), dim3(256), 0, ctx->stream, d_values, (long long)n, part_p);
    HIP_TRY(hipGetLastError());
    std::vector<float> h(blocks);
    HIP_TRY(hipMemcpyAsync(h.data(), part_p, (size_t)blocks * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    float m = h[0];
    for (int i = 1; i < blocks; i++)
        m = std::max(m, h[i]);
    *h_max = m;
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_f2c_tighten_bounds(rslf_ctx* ctx, const float* d_depth_up_svu, const uint8_t* d_valid_up_svu, int S, int V_up,
                                       int U_up, float* d_dmin_down_svu, float* d_dmax_down_svu, int V_down, int U_down) RSLF_API_TRY
{
    if (!ctx || !d_depth_up_svu || !d_valid_up_svu || !d_dmin_down_svu || !d_dmax_down_svu || S < 1 || V_up < 1 || U_up < 1 ||
        V_down < 1 || U_down < 1)
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n_up = (size_t)S * V_up * U_up;
    void *left_p = nullptr, *right_p = nullptr;
    int rc = helper_scratch(ctx, kSharedLeft, n_up * sizeof(int), &left_p);
    if (!rc)
        rc = helper_scratch(ctx, kSharedRight, n_up * sizeof(int), &right_p);
    if (rc)
        return rc;
    hipStream_t st = ctx->stream;
    const long long rows = (long long)S * V_up;
    hipLaunchKernelGGL(k5_nearest_valid, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, d_valid_up_svu, rows, U_up,
                       (int*)left_p, (int*)right_p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k5_tighten, dim3((U_down + 255) / 256, V_down, S), dim3(256), 0, st, d_depth_up_svu, (const int*)left_p,
                       (const int*)right_p, S, V_up, U_up, d_dmin_down_svu, d_dmax_down_svu, V_down, U_down);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;   // enqueued, not awaited
}
RSLF_API_CATCH

extern "C" int rslf_f2c_fuse(rslf_ctx* ctx, const float* const* d_disp, const uint8_t* const* d_valid, const int* Vp, const int* Up,
                             int P, int S, float* d_out_map_svu, uint8_t* d_out_valid_svu) RSLF_API_TRY
{
    if (!ctx || !d_disp || !d_valid || !Vp || !Up || P < 1 || S < 1 || !d_out_map_svu || !d_out_valid_svu)
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n0 = (size_t)S * Vp[0] * Up[0];
    // two ping-pong buffers at the finest size hold the running map / mask of every step
    void *mapA = nullptr, *mapB = nullptr, *mskA = nullptr, *mskB = nullptr;
    int rc = helper_scratch(ctx, kSharedLevel, n0 * sizeof(float), &mapA);
    if (!rc)
        rc = helper_scratch(ctx, kSharedLeft, n0 * sizeof(float), &mapB);
    if (!rc)
        rc = helper_scratch(ctx, kSharedTable, n0, &mskA);
    if (!rc)
        rc = helper_scratch(ctx, kSharedRight, n0, &mskB);
    if (rc)
        return rc;
    float* map_down = (float*)mapA;
    float* map_next = (float*)mapB;
    uint8_t* msk_down = (uint8_t*)mskA;
    uint8_t* msk_next = (uint8_t*)mskB;
    const size_t nl = (size_t)S * Vp[P - 1] * Up[P - 1];
    HIP_TRY(hipMemcpyAsync(map_down, d_disp[P - 1], nl * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(msk_down, d_valid[P - 1], nl, hipMemcpyDeviceToDevice, st));
    for (int p = P - 1; p > 0; p--) {   // fine_to_coarse_core.cpp:98-123
        const int R = Vp[p], W = Up[p], R2 = Vp[p - 1], W2 = Up[p - 1];
        hipLaunchKernelGGL(k5_fuse_step, dim3((W2 + 255) / 256, R2, S), dim3(256), 0, st, map_down, msk_down, R, W, d_disp[p - 1],
                           d_valid[p - 1], map_next, msk_next, R2, W2);
        HIP_TRY(hipGetLastError());
        std::swap(map_down, map_next);
        std::swap(msk_down, msk_next);
    }
    hipLaunchKernelGGL(k5_median3, dim3((Up[0] + 255) / 256, Vp[0], S), dim3(256), 0, st, map_down, d_out_map_svu, Vp[0], Up[0]);   // :127
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(d_out_valid_svu, msk_down, n0, hipMemcpyDeviceToDevice, st));
    return RSLF_OK;   // enqueued, not awaited
}
RSLF_API_CATCH

namespace {
template <typename T>
__global__ __launch_bounds__(256) void k_to_f32(const T* __restrict__ in, float* __restrict__ out, long long n)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = (float)in[i];
}
__global__ __launch_bounds__(256) void k_fill_f32(float* __restrict__ out, long long n, float value)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = value;
}
// get_valid_depths_mask_s_v_u (dc.hpp:893-915): a confidence plane > thr -- C_e, or C_l / C_d where
// plan::f2c_validity_by_rule says so; everything (C_e > -1) with accept_all
__global__ __launch_bounds__(256) void k_valid_mask(const float* __restrict__ conf, uint8_t* __restrict__ out, long long n, float thr)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = (conf[i] > thr) ? 255 : 0;
}
inline unsigned stream_blocks(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 8192); }
}  // namespace

// The finest level's raw values from host EPIs of element type e into the dense float volume d_raw [V][S][U][C] (integer
// types widened on the device); synchronises.
static int f2c_upload_raw(rslf_ctx* ctx, Elem e, const void* const* h_epis, int V, int S, int U, int C, size_t row_stride_bytes,
                          float* d_raw)
{
    hipStream_t st = ctx->stream;
    const size_t row_bytes = (size_t)U * C * elem_bytes(e);
    if (row_stride_bytes == 0)
        row_stride_bytes = row_bytes;
    if (row_stride_bytes < row_bytes)
        return fail(RSLF_ERR_INVALID_ARG, "row_stride_bytes %zu < row size %zu", row_stride_bytes, row_bytes);
    for (int v = 0; v < V; v++)
        if (!h_epis[v])
            return fail(RSLF_ERR_INVALID_ARG, "h_epis[%d] is NULL", v);
    DevBuf stage;   // integer EPIs go up as they are and are widened on the device
    void* dst = d_raw;
    if (e != Elem::F32) {
        HIP_TRY(stage.alloc((size_t)V * S * row_bytes));
        dst = stage.get();
    }
    for (int v = 0; v < V; v++) {
        if (row_stride_bytes == row_bytes)   // dense rows: one run of bytes per EPI (upload_host)
            HIP_TRY(hipMemcpyAsync((char*)dst + (size_t)v * S * row_bytes, h_epis[v], (size_t)S * row_bytes, hipMemcpyHostToDevice, st));
        else
            HIP_TRY(hipMemcpy2DAsync((char*)dst + (size_t)v * S * row_bytes, row_bytes, h_epis[v], row_stride_bytes, row_bytes, S,
                                     hipMemcpyHostToDevice, st));
    }
    const size_t n = (size_t)V * S * U * C;
    if (e == Elem::U8)
        hipLaunchKernelGGL(k_to_f32<uint8_t>, dim3(stream_blocks(n)), dim3(256), 0, st, stage.as<const uint8_t>(), d_raw, (long long)n);
    else if (e == Elem::U16)
        hipLaunchKernelGGL(k_to_f32<uint16_t>, dim3(stream_blocks(n)), dim3(256), 0, st, stage.as<const uint16_t>(), d_raw, (long long)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (the staging buffer is freed on return)
    return RSLF_OK;
}
// The level rule of FineToCoarse on element type e: the level's epi_scale_factor (CV_8U: 255; otherwise the given factor or,
// when < 0, the level's own max -- dc.hpp:671-705) and the halving that keeps the Mats' type (f2c_downsample).
static int f2c_level_scale(rslf_ctx* ctx, Elem e, const float* d_raw, size_t n, float epi_scale_factor, float* scale)
{
    if (e == Elem::U8) {   // dc.hpp:696-699 (uchar)
        *scale = 255.0f;
        return RSLF_OK;
    }
    *scale = epi_scale_factor;
    if (*scale < 0)        // dc.hpp:671-690: this level's own max
        return rslf_device_max_f32(ctx, d_raw, n, scale);
    return RSLF_OK;
}
static int f2c_downsample(rslf_ctx* ctx, Elem e, const float* d_in_vsuc, int V, int S, int U, int C, float* d_out_vsuc)
{
    // integer EPIs go down in their own arithmetic, as the reference's Mats do (fine_to_coarse_core.cpp:22-41)
    switch (e) {
    case Elem::U8:
        return rslf_downsample_epis_u8(ctx, d_in_vsuc, V, S, U, C, d_out_vsuc);
    case Elem::U16:
        return rslf_downsample_epis_u16(ctx, d_in_vsuc, V, S, U, C, d_out_vsuc);
    default:
        return rslf_downsample_epis_f32(ctx, d_in_vsuc, V, S, U, C, d_out_vsuc);
    }
}
static int f2c_fill_f32(hipStream_t st, float* out, size_t n, float value)
{
    hipLaunchKernelGGL(k_fill_f32, dim3(stream_blocks(n)), dim3(256), 0, st, out, (long long)n, value);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}
static int f2c_valid_mask(hipStream_t st, const float* conf, uint8_t* out, size_t n, float thr)
{
    hipLaunchKernelGGL(k_valid_mask, dim3(stream_blocks(n)), dim3(256), 0, st, conf, out, (long long)n, thr);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

// The level dilation runs the sweeps' frame alone; K7 samples C_e along u + (s_hat - s) * d with no slope factor.
int rslf::check_level_dilation(const F2cOptions& o)
{
    if (!dilate_factor_ok(o.level_dilation))
        return fail(RSLF_ERR_INVALID_ARG, "level_dilation=%d: an integer in 1..%d", o.level_dilation, kDilateMaxFactor);
    if (!dilate_kind_ok(o.dilation_kind))
        return fail(RSLF_ERR_INVALID_ARG, "dilation_kind=%d: RSLF_DILATE_LINEAR, RSLF_DILATE_CUBIC or RSLF_DILATE_LANCZOS3", o.dilation_kind);
    if (o.level_dilation > 1 && o.line_mode != RSLF_LINE_CONF_OFF)
        return fail(RSLF_ERR_UNSUPPORTED, "level_dilation=%d together with line confidence mode %d is not built (the line confidence "
                    "takes no slope factor)", o.level_dilation, o.line_mode);
    return RSLF_OK;
}

int rslf::fine_to_coarse(rslf_ctx* ctx, const F2cRequest& req, const F2cOptions& o, const F2cHostOut& out, rslf_stats* stats,
                         F2cKept* keep, const std::function<int(const F2cLevel& level, rslf_stats* level_stats)>& sweep)
{
    const int V = req.V, S = req.S, U = req.U;
    const rslf_params* const p = req.p;
    if (!ctx || !req.h_epis || V < 1 || S < 1 || U < 1 || (req.C != 1 && req.C != 3))
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    // the derivative channels (K17): a one-channel field is (x, |dx/du|, |dx/dv|) from its upload on, and everything below
    // runs as it does for a three-channel field
    if (!plan::derivative_option_ok(o.derivative_weight))
        return fail(RSLF_ERR_INVALID_ARG, "derivative_weight=%g: 0 (off) or a finite weight > 0", (double)o.derivative_weight);
    const bool derivative = o.derivative_weight > 0.0f;
    if (derivative && req.C != 1)
        return fail(RSLF_ERR_UNSUPPORTED, "derivative_weight=%g with C=%d: the derivative channels are built for a one-channel field",
                    (double)o.derivative_weight, req.C);
    const int C = derivative ? kDerivativeChannels : req.C;
    if (!keep && (!out.map_svu || !out.valid_svu))   // a kept run holds the fused planes itself
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    if (!plan::f2c_validity_rule_ok(o.validity_rule) || (!keep && o.validity_rule != RSLF_F2C_VALID_COMPAT))
        return fail(RSLF_ERR_INVALID_ARG, "validity rule %d: RSLF_F2C_VALID_COMPAT or, for a kept run, _REFERENCE", o.validity_rule);
    if (!plan::line_conf_mode_ok(o.line_mode))
        return fail(RSLF_ERR_INVALID_ARG, "line confidence mode %d: must be RSLF_LINE_CONF_OFF, _AS_BUILT or _GATE", o.line_mode);
    if (int rc = check_level_dilation(o))
        return rc;
    if (int rc = check_equalize(o, V, S, U, req.C))
        return rc;
    int rc = check_params(p);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // constructor: rslf_fine_to_coarse.hpp:103-159 -- the level sizes are plan::f2c_pyramid
    const std::vector<plan::LevelDims> dims = plan::f2c_pyramid(V, U, req.max_pyr_depth);
    if (dims.empty())
        return fail(RSLF_ERR_INVALID_ARG, "light field %dx%d is not larger than _MIN_SPATIAL_DIM: no pyramid level", V, U);
    const int P = (int)dims.size();
    if (out.levels && out.levels->capacity < P)
        return fail(RSLF_ERR_INVALID_ARG, "levels out: capacity %d < pyramid depth %d", out.levels->capacity, P);
    DevBuf raw;   // the raw (un-normalised) values of the level at hand, [V][S][U][C]
    HIP_TRY(raw.alloc((size_t)V * S * U * req.C * sizeof(float)));
    rc = f2c_upload_raw(ctx, req.elem, req.h_epis, V, S, U, req.C, req.row_stride_bytes, raw.as<float>());
    if (rc)
        return rc;
    // the per-view equalisation (K19): once, in place, on the finest level's upload; everything below -- the derivative
    // channels first -- reads the equalised intensity
    std::vector<float> view_gains;
    if (o.equalize_mode != 0) {
        float hi = 0.0f;   // (integer elements: their type's, equalize_views_raw)
        if (req.elem == Elem::F32) {
            rc = rslf_device_max_f32(ctx, raw.as<const float>(), (size_t)V * S * U * req.C, &hi);
            if (rc)
                return rc;
            if (!eq_hi_ok(hi))
                return fail(RSLF_ERR_UNSUPPORTED, "equalize_views=%d on a float field whose maximum is %g: the cap is finite and > 0",
                            o.equalize_mode, (double)hi);
        }
        view_gains.resize((size_t)S * req.C * 2);
        rc = equalize_views_raw(ctx, raw.as<float>(), req.elem, V, S, U, req.C, hi, o.equalize_mode, o.equalize_ref_view, o.equalize_joint,
                                o.equalize_max_gain, view_gains.data());
        if (rc)
            return rc;
    }
    if (derivative) {   // once, at the finest level: the features go down with the intensity from here
        float hi = 0.0f;   // (integer elements: their type's, derivative_channels_raw)
        if (req.elem == Elem::F32) {
            rc = rslf_device_max_f32(ctx, raw.as<const float>(), (size_t)V * S * U, &hi);
            if (rc)
                return rc;
            hi = derivative_hi_f32(hi);
        }
        DevBuf source;
        std::swap(raw, source);
        HIP_TRY(raw.alloc((size_t)V * S * U * C * sizeof(float)));
        rc = derivative_channels_raw(ctx, source.as<const float>(), req.elem, V, S, U, o.derivative_weight, hi, raw.as<float>());
        if (rc)
            return rc;
    }   // (`source` is freed here, which waits for the device)

    // run(): rslf_fine_to_coarse.hpp:171-299, each level built just before its sweep; every level keeps its disparities
    // and validity for the fusion -- and everything else where the caller owns the planes
    F2cKept own;
    F2cKept& K = keep ? *keep : own;
    K.levels = std::vector<F2cKeptLevel>((size_t)P);
    K.view_gains = std::move(view_gains);
    int64_t pixels = 0;
    rslf_stats st1;
    memset(&st1, 0, sizeof(st1));
    DevBuf cs_dropped;   // the consistency gate's counters, one per level: zeroed here, read once after the loop's last wait
    if (o.cs_min_agree > 0) {
        HIP_TRY(cs_dropped.alloc((size_t)P * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(cs_dropped.get(), 0, (size_t)P * sizeof(unsigned long long), st));
    }
    for (int l = 0; l < P; l++) {
        F2cKeptLevel& kl = K.levels[(size_t)l];
        F2cLevel lv;
        lv.V = kl.V = dims[l].V;
        lv.U = kl.U = dims[l].U;
        lv.C = C;
        lv.params = *p;
        lv.params.slope_factor = (float)((0.0 + lv.U) / U);              // f2c.hpp:139
        kl.slope = lv.params.slope_factor;
        const size_t n = (size_t)S * lv.V * lv.U;
        rc = f2c_level_scale(ctx, req.elem, raw.as<const float>(), n * C, req.epi_scale_factor, &lv.scale);
        if (rc)
            return rc;
        kl.scale = lv.scale;
        DevBuf next;                                                       // f2c.hpp:145-147: the RAW EPIs go down
        if (l + 1 < P) {
            HIP_TRY(next.alloc((size_t)dims[l + 1].V * S * dims[l + 1].U * C * sizeof(float)));
            rc = f2c_downsample(ctx, req.elem, raw.as<const float>(), lv.V, S, lv.U, C, next.as<float>());
            if (rc)
                return rc;
        }
        DevBuf dmin, dmax, ungated;   // (ungated: the validity the consistency gate read, freed with the level's ranges)
        DevBuf &Ce = kl.Ce, &Cl = kl.Cl;
        HIP_TRY(Ce.alloc(n * 4));
        if (o.line_mode != RSLF_LINE_CONF_OFF)
            HIP_TRY(Cl.alloc(n * 4));   // dc.hpp:721-738: every level's computer has a plane of its own
        HIP_TRY(kl.depth.alloc(n * 4));
        HIP_TRY(kl.valid.alloc(n));
        if (keep)
            HIP_TRY(kl.Cd.alloc(n * 4));
        rslf_peaks pk = {};
        if (o.peaks) {   // the level's sweep fills them with -1 / 0 before its first visit (depth2d_run)
            HIP_TRY(kl.pk_idx.alloc(n * 4));
            HIP_TRY(kl.pk_score.alloc(n * 4));
            HIP_TRY(kl.pk_runner_idx.alloc(n * 4));
            HIP_TRY(kl.pk_runner_score.alloc(n * 4));
            pk.idx = kl.pk_idx.as<int32_t>();
            pk.score = kl.pk_score.as<float>();
            pk.runner_idx = kl.pk_runner_idx.as<int32_t>();
            pk.runner_score = kl.pk_runner_score.as<float>();
            lv.peaks = &pk;
            lv.withheld = &kl.withheld;
        }
        if (l > 0) {
            HIP_TRY(dmin.alloc(n * 4));
            HIP_TRY(dmax.alloc(n * 4));
            rc = f2c_fill_f32(st, dmin.as<float>(), n, req.d_min);
            if (!rc)
                rc = f2c_fill_f32(st, dmax.as<float>(), n, req.d_max);
            if (!rc)
                rc = rslf_f2c_tighten_bounds(ctx, K.levels[(size_t)l - 1].depth.as<const float>(),
                                             K.levels[(size_t)l - 1].valid.as<const uint8_t>(), S, dims[l - 1].V, dims[l - 1].U,
                                             dmin.as<float>(), dmax.as<float>(), lv.V, lv.U);
            if (rc)
                return rc;
        }
        lv.raw_vsuc = raw.as<const float>();
        lv.dmin_svu = dmin.as<const float>();
        lv.dmax_svu = dmax.as<const float>();
        lv.Ce_svu = Ce.as<float>();
        lv.depth_svu = kl.depth.as<float>();
        lv.options = &o;
        lv.Cl_svu = Cl.as<float>();
        lv.Cd_svu = kl.Cd.as<float>();
        lv.vol_out = (keep && o.keep_volumes) ? &kl.vol : nullptr;
        rc = sweep(lv, &st1);
        if (rc)
            return rc;
        pixels += st1.pixels_scanned;
        // get_valid_depths_mask_s_v_u (dc.hpp:893-915), asked for by the next level's bounds (f2c.hpp:185-186) and by the
        // fusion (:312): the last level accepts everything when asked to (f2c.hpp:157-158)
        const plan::F2cValidity by = plan::f2c_validity_by_rule(req.accept_all_last_scale && l == P - 1, p->use_disp_confidence_score != 0,
                                                                o.line_mode, o.validity_rule);
        switch (by) {
        case plan::kValidAll:
            rc = f2c_valid_mask(st, Ce.as<const float>(), kl.valid.as<uint8_t>(), n, -1.0f);
            break;
        case plan::kValidLineConf:
            rc = f2c_valid_mask(st, Cl.as<const float>(), kl.valid.as<uint8_t>(), n, p->line_score_threshold);
            break;
        case plan::kValidEdgeConf:
            rc = f2c_valid_mask(st, Ce.as<const float>(), kl.valid.as<uint8_t>(), n, p->edge_score_threshold);
            break;
        case plan::kValidDispConf:   // the REFERENCE rule alone, so a kept run: C_d is the owner's (dc.hpp:902)
            rc = f2c_valid_mask(st, kl.Cd.as<const float>(), kl.valid.as<uint8_t>(), n, p->disp_score_threshold);
            break;
        }
        // validity by uniqueness: what the rule left valid goes invalid where the runner-up is within the ratio of the winner
        if (!rc && o.peaks && plan::f2c_unique_applies(o.uniqueness, by))
            rc = rslf_f2c_unique_mask(ctx, kl.valid.as<uint8_t>(), &pk, o.uniqueness, n);
        // validity by cross-view consistency: what is still valid goes invalid where the other views contradict it.  The gate
        // writes a second plane (a thread reads the other views' rows while they are written), which takes the first one's place
        if (!rc && plan::f2c_consistency_applies(o.cs_min_agree, by)) {
            HIP_TRY(ungated.alloc(n));
            HIP_TRY(kl.cs_agree.alloc(n * 4));
            HIP_TRY(kl.cs_seen.alloc(n * 4));
            rc = rslf_f2c_consistency_mask(ctx, kl.depth.as<const float>(), kl.valid.as<const uint8_t>(), S, lv.V, lv.U, kl.slope, o.cs_tol,
                                           o.cs_radius, o.cs_min_agree, ungated.as<uint8_t>(), kl.cs_agree.as<int32_t>(),
                                           kl.cs_seen.as<int32_t>(), cs_dropped.as<unsigned long long>() + l);
            std::swap(kl.valid, ungated);   // kl.valid: the gated plane
        }
        if (rc)
            return rc;
        if (out.levels) {   // host copies of the level's planes; C_e and C_l leave the device with this iteration
            const auto copy = [&](void* const* hp, const void* d, size_t bytes) -> hipError_t {
                return (hp && hp[l] && d) ? hipMemcpyAsync(hp[l], d, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
            };
            HIP_TRY(copy((void* const*)out.levels->h_depth_svu, kl.depth.get(), n * 4));
            HIP_TRY(copy((void* const*)out.levels->h_valid_svu, kl.valid.get(), n));
            HIP_TRY(copy((void* const*)out.levels->h_Cl_svu, Cl.get(), n * 4));
            HIP_TRY(copy((void* const*)out.levels->h_Ce_svu, Ce.get(), n * 4));
            HIP_TRY(hipStreamSynchronize(st));
        }
        if (!keep) {            // the level's confidences have served
            Cl.release();
            Ce.release();
        }
        std::swap(raw, next);   // `next` now frees this level's raw volume
    }

    // get_results(): rslf_fine_to_coarse.hpp:302-324
    std::vector<const float*> dp(P);
    std::vector<const uint8_t*> vp(P);
    std::vector<int> Vp(P), Up(P);
    for (int l = 0; l < P; l++) {
        dp[l] = K.levels[(size_t)l].depth.as<const float>();
        vp[l] = K.levels[(size_t)l].valid.as<const uint8_t>();
        Vp[l] = dims[l].V;
        Up[l] = dims[l].U;
    }
    const size_t n0 = (size_t)S * V * U;
    DevBuf &omap = K.fused_map, &ovalid = K.fused_valid;
    HIP_TRY(omap.alloc(n0 * 4));
    HIP_TRY(ovalid.alloc(n0));
    rc = rslf_f2c_fuse(ctx, dp.data(), vp.data(), Vp.data(), Up.data(), P, S, omap.as<float>(), ovalid.as<uint8_t>());
    if (rc)
        return rc;
    if (o.peaks) {   // which level decided each fused pixel, and that level's peaks there: one launch over the whole pyramid
        std::vector<rslf_peaks> pp((size_t)P);
        for (int l = 0; l < P; l++) {
            F2cKeptLevel& kl = K.levels[(size_t)l];
            pp[(size_t)l] = rslf_peaks{kl.pk_idx.as<int32_t>(), kl.pk_score.as<float>(), nullptr, kl.pk_runner_idx.as<int32_t>(),
                                       kl.pk_runner_score.as<float>()};
        }
        HIP_TRY(K.fused_pk_idx.alloc(n0 * 4));
        HIP_TRY(K.fused_pk_score.alloc(n0 * 4));
        HIP_TRY(K.fused_pk_runner_idx.alloc(n0 * 4));
        HIP_TRY(K.fused_pk_runner_score.alloc(n0 * 4));
        HIP_TRY(K.fused_level.alloc(n0));
        const rslf_peaks fused = {K.fused_pk_idx.as<int32_t>(), K.fused_pk_score.as<float>(), nullptr,
                                  K.fused_pk_runner_idx.as<int32_t>(), K.fused_pk_runner_score.as<float>()};
        rc = rslf_f2c_fuse_peaks(ctx, vp.data(), pp.data(), Vp.data(), Up.data(), P, S, &fused, K.fused_level.as<uint8_t>());
        if (rc)
            return rc;
    }
    if (out.map_svu)
        HIP_TRY(hipMemcpyAsync(out.map_svu, omap.get(), n0 * 4, hipMemcpyDeviceToHost, st));
    if (out.valid_svu)
        HIP_TRY(hipMemcpyAsync(out.valid_svu, ovalid.get(), n0, hipMemcpyDeviceToHost, st));
    std::vector<unsigned long long> dropped((size_t)P, 0ull);
    if (o.cs_min_agree > 0)
        HIP_TRY(hipMemcpyAsync(dropped.data(), cs_dropped.get(), (size_t)P * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int l = 0; l < P; l++)
        K.levels[(size_t)l].inconsistent = dropped[(size_t)l];
    if (out.n_levels)
        *out.n_levels = P;
    if (stats) {
        *stats = st1;
        stats->pixels_scanned = pixels;
        stats->units = pixels * req.dim_d;
    }
    return RSLF_OK;
}

// FineToCoarse on one context: each level a volume of its own, packed from the raw level and swept by depth2d_run.
int rslf::fine_to_coarse_one_context(rslf_ctx* ctx, const F2cRequest& req, const F2cOptions& o, const F2cHostOut& out,
                                     rslf_stats* stats, F2cKept* keep)
{
    SweepModes asked;   // what of the levels' modes can be refused before the loop allocates: the planes come with each level
    asked.subgrid = o.subgrid;
    if (int rc = check_sweep_modes(asked))
        return rc;
    const int S = req.S;
    auto sweep = [&](const F2cLevel& lv, rslf_stats* level_stats) -> int {
        if (inject_hit(kInjectSweep))   // host side, before the level's sweep is queued
            throw std::runtime_error("injected failure in a fine-to-coarse level (rslf_debug_inject)");
        const int f = o.level_dilation;
        int Ud = lv.U;   // the width of the sweep's frame: U' = f (U_l - 1) + 1 with the level dilation, else the level's
        if (f > 1 && plan::dilated_width(lv.U, f, &Ud) != plan::kDilateOk)
            return fail(RSLF_ERR_UNSUPPORTED, "U=%d dilated by %d does not fit a row", lv.U, f);
        const size_t rows = (size_t)S * lv.V;
        const size_t n = rows * Ud;
        const int C = lv.C;   // (the request's, or 3 with the derivative channels)
        DevBuf Cd, rbar, mask;
        if (!lv.Cd_svu || f > 1)   // a kept run's C_d is its owner's (on the level's grid)
            HIP_TRY(Cd.alloc(n * 4));
        HIP_TRY(rbar.alloc(n * 4 * C));
        HIP_TRY(mask.alloc(n));
        VolumePtr vol;
        rslf_volume* made = nullptr;
        int rc = rslf_volume_create(ctx, lv.V, S, lv.U, C, &made);
        vol.reset(made);
        if (!rc)
            rc = rslf_volume_pack_device_f32(vol.get(), lv.raw_vsuc, lv.scale, nullptr);
        SweepModes modes;
        modes.line_mode = o.line_mode, modes.Cl_svu = lv.Cl_svu, modes.subgrid = o.subgrid;
        modes.peaks = lv.peaks, modes.propagation_ratio = o.propagation_ratio;
        if (f > 1) {
            // The level dilation: the sweep alone runs in the dilated frame.  Its volume is the level's packed volume dilated
            // (K16; the clamp range is the packed volume's), its ranges the level's by the union rule (K18), its slope factor the
            // level's times f in one binary32 product; the planes the loop reads are the columns u * f of the sweep's.
            VolumePtr vol_d;
            rslf_volume* dilated = nullptr;
            if (!rc)
                rc = rslf_volume_dilate_u(ctx, vol.get(), f, o.dilation_kind, &dilated);
            vol_d.reset(dilated);
            DevBuf Ce_d, depth_d, dmin_d, dmax_d, pk_d[4];
            HIP_TRY(Ce_d.alloc(n * 4));
            HIP_TRY(depth_d.alloc(n * 4));
            if (lv.dmin_svu) {
                HIP_TRY(dmin_d.alloc(n * 4));
                HIP_TRY(dmax_d.alloc(n * 4));
                if (!rc)
                    rc = rslf_planes_dilate_ranges_u(ctx, lv.dmin_svu, lv.dmax_svu, rows, lv.U, f, dmin_d.as<float>(), dmax_d.as<float>());
            }
            rslf_peaks pk_planes = {};
            if (lv.peaks) {
                for (DevBuf& b : pk_d)
                    HIP_TRY(b.alloc(n * 4));
                pk_planes = rslf_peaks{pk_d[0].as<int32_t>(), pk_d[1].as<float>(), nullptr, pk_d[2].as<int32_t>(), pk_d[3].as<float>()};
                modes.peaks = &pk_planes;
            }
            rslf_params params = lv.params;
            params.slope_factor = lv.params.slope_factor * (float)f;   // (no contraction: one product, rounded once)
            const SweepPlanes planes = {Ce_d.as<float>(), mask.as<uint8_t>(), Cd.as<float>(), depth_d.as<float>(), rbar.as<float>(), nullptr};
            if (!rc)
                rc = depth2d_run(ctx, vol_d.get(), lv.dmin_svu ? dmin_d.as<const float>() : nullptr, lv.dmin_svu ? dmax_d.as<const float>() : nullptr,
                                 req.d_min, req.d_max, req.dim_d, &params, planes, level_stats, modes);
            if (!rc && o.propagation_ratio > 0.0f && lv.withheld)
                rc = rslf_sweep_withheld(ctx, lv.withheld);
            // back to the level's grid in one launch: depth, C_e, C_d (a kept run's) and the four peak planes
            const void* in[8];
            void* back[8];
            int bytes[8], np = 0;
            const auto add = [&](const void* from, void* to) {
                if (to)
                    in[np] = from, back[np] = to, bytes[np] = 4, ++np;
            };
            add(depth_d.get(), lv.depth_svu);
            add(Ce_d.get(), lv.Ce_svu);
            add(Cd.get(), lv.Cd_svu);
            if (lv.peaks) {
                add(pk_d[0].get(), lv.peaks->idx);
                add(pk_d[1].get(), lv.peaks->score);
                add(pk_d[2].get(), lv.peaks->runner_idx);
                add(pk_d[3].get(), lv.peaks->runner_score);
            }
            if (!rc)
                rc = rslf_planes_undilate_many_u(ctx, in, back, bytes, np, rows, Ud, f);
            if (!rc && lv.vol_out)
                *lv.vol_out = std::move(vol);   // the undilated level; the dilated volume and the sweep's planes are destroyed here
            return rc;
        }
        const SweepPlanes planes = {lv.Ce_svu, mask.as<uint8_t>(), lv.Cd_svu ? lv.Cd_svu : Cd.as<float>(), lv.depth_svu, rbar.as<float>(),
                                    nullptr};
        if (!rc)
            rc = depth2d_run(ctx, vol.get(), lv.dmin_svu, lv.dmax_svu, req.d_min, req.d_max, req.dim_d, &lv.params, planes, level_stats, modes);
        if (!rc && o.propagation_ratio > 0.0f && lv.withheld)
            rc = rslf_sweep_withheld(ctx, lv.withheld);
        if (!rc && lv.vol_out)
            *lv.vol_out = std::move(vol);   // kept; otherwise destroyed here, with the sweep's other planes
        return rc;
    };
    return fine_to_coarse(ctx, req, o, out, stats, keep, sweep);
}

extern "C" int rslf_f2c_pyramid_dims(int V, int U, int max_pyr_depth, int* Vp, int* Up, int capacity, int* n_levels) RSLF_API_TRY
{
    if (!n_levels || V < 1 || U < 1 || capacity < 0 || (capacity > 0 && (!Vp || !Up)))
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    const std::vector<plan::LevelDims> dims = plan::f2c_pyramid(V, U, max_pyr_depth);
    *n_levels = (int)dims.size();
    if (capacity < *n_levels)
        return capacity == 0 ? RSLF_OK : fail(RSLF_ERR_INVALID_ARG, "capacity %d < pyramid depth %d", capacity, *n_levels);
    for (int l = 0; l < *n_levels; l++) {
        Vp[l] = dims[l].V;
        Up[l] = dims[l].U;
    }
    return RSLF_OK;
}
RSLF_API_CATCH

// The host-planes entries: the same call, the request in the order of their arguments; what an entry lacks stays off.

extern "C" int rslf_fine_to_coarse_run_host(rslf_ctx* ctx, const void* const* h_epis, int is_u8, int V, int S, int U, int C,
                                            size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                            const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                            float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats) RSLF_API_TRY
{
    const F2cRequest req = {is_u8 ? Elem::U8 : Elem::F32, h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p,
                            max_pyr_depth, accept_all_last_scale};
    return fine_to_coarse_one_context(ctx, req, F2cOptions(), {h_out_map_svu, h_out_valid_svu, n_levels, nullptr}, stats, nullptr);
}
RSLF_API_CATCH

extern "C" int rslf_fine_to_coarse_run_host_u16(rslf_ctx* ctx, const uint16_t* const* h_epis, int V, int S, int U, int C,
                                                size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                                const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                                float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats) RSLF_API_TRY
{
    const F2cRequest req = {Elem::U16, (const void* const*)h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p,
                            max_pyr_depth, accept_all_last_scale};
    return fine_to_coarse_one_context(ctx, req, F2cOptions(), {h_out_map_svu, h_out_valid_svu, n_levels, nullptr}, stats, nullptr);
}
RSLF_API_CATCH

extern "C" int rslf_fine_to_coarse_run_host_lc(rslf_ctx* ctx, const void* const* h_epis, int is_u8, int V, int S, int U, int C,
                                               size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                               const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                               float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats,
                                               int line_mode, const rslf_f2c_levels_out* levels_out) RSLF_API_TRY
{
    const F2cRequest req = {is_u8 ? Elem::U8 : Elem::F32, h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p,
                            max_pyr_depth, accept_all_last_scale};
    F2cOptions options;
    options.line_mode = line_mode;
    return fine_to_coarse_one_context(ctx, req, options, {h_out_map_svu, h_out_valid_svu, n_levels, levels_out}, stats, nullptr);
}
RSLF_API_CATCH

extern "C" int rslf_fine_to_coarse_run_host_u16_lc(rslf_ctx* ctx, const uint16_t* const* h_epis, int V, int S, int U, int C,
                                                   size_t row_stride_bytes, float d_min, float d_max, int dim_d,
                                                   float epi_scale_factor, const rslf_params* p, int max_pyr_depth,
                                                   int accept_all_last_scale, float* h_out_map_svu, uint8_t* h_out_valid_svu,
                                                   int* n_levels, rslf_stats* stats, int line_mode,
                                                   const rslf_f2c_levels_out* levels_out) RSLF_API_TRY
{
    const F2cRequest req = {Elem::U16, (const void* const*)h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p,
                            max_pyr_depth, accept_all_last_scale};
    F2cOptions options;
    options.line_mode = line_mode;
    return fine_to_coarse_one_context(ctx, req, options, {h_out_map_svu, h_out_valid_svu, n_levels, levels_out}, stats, nullptr);
}
RSLF_API_CATCH

// ... any element type (RSLF_ELEM_*), every level's sweep in the sub-grid mode with subgrid = 1
extern "C" int rslf_fine_to_coarse_run_host_sub(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C,
                                                size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                                const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                                float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats,
                                                int line_mode, const rslf_f2c_levels_out* levels_out, int subgrid) RSLF_API_TRY
{
    Elem e;
    if (int rc = elem_of(elem, &e))
        return rc;
    const F2cRequest req = {e, h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p, max_pyr_depth,
                            accept_all_last_scale};
    F2cOptions options;
    options.line_mode = line_mode, options.subgrid = subgrid;
    return fine_to_coarse_one_context(ctx, req, options, {h_out_map_svu, h_out_valid_svu, n_levels, levels_out}, stats, nullptr);
}
RSLF_API_CATCH

// ... and with derivative_weight > 0 a one-channel field goes down the pyramid as (x, |dx/du|, |dx/dv|) (K17)
extern "C" int rslf_fine_to_coarse_run_host_dv(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C,
                                               size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                               const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                               float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats,
                                               int line_mode, const rslf_f2c_levels_out* levels_out, int subgrid,
                                               float derivative_weight) RSLF_API_TRY
{
    Elem e;
    if (int rc = elem_of(elem, &e))
        return rc;
    const F2cRequest req = {e, h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p, max_pyr_depth,
                            accept_all_last_scale};
    F2cOptions options;
    options.line_mode = line_mode, options.subgrid = subgrid, options.derivative_weight = derivative_weight;
    return fine_to_coarse_one_context(ctx, req, options, {h_out_map_svu, h_out_valid_svu, n_levels, levels_out}, stats, nullptr);
}
RSLF_API_CATCH

// ... and with level_dilation > 1 every level's sweep runs on the level's volume dilated along u (K16) and its planes come
// back to the level's own grid (K18); 1: the narrower entry's call
extern "C" int rslf_fine_to_coarse_run_host_dl(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C,
                                               size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                               const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                               float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats,
                                               int line_mode, const rslf_f2c_levels_out* levels_out, int subgrid,
                                               float derivative_weight, int level_dilation, int dilation_kind) RSLF_API_TRY
{
    Elem e;
    if (int rc = elem_of(elem, &e))
        return rc;
    const F2cRequest req = {e, h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p, max_pyr_depth,
                            accept_all_last_scale};
    F2cOptions options;
    options.line_mode = line_mode, options.subgrid = subgrid, options.derivative_weight = derivative_weight;
    options.level_dilation = level_dilation, options.dilation_kind = dilation_kind;
    return fine_to_coarse_one_context(ctx, req, options, {h_out_map_svu, h_out_valid_svu, n_levels, levels_out}, stats, nullptr);
}
RSLF_API_CATCH

// ... and with equalize_mode != 0 the finest level's upload is equalised per view, in place, before anything reads it (K19)
extern "C" int rslf_fine_to_coarse_run_host_eq(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C,
                                               size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                               const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                               float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats,
                                               int line_mode, const rslf_f2c_levels_out* levels_out, int subgrid,
                                               float derivative_weight, int level_dilation, int dilation_kind, int equalize_mode,
                                               int equalize_ref_view, int equalize_joint, float equalize_max_gain) RSLF_API_TRY
{
    Elem e;
    if (int rc = elem_of(elem, &e))
        return rc;
    const F2cRequest req = {e, h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p, max_pyr_depth,
                            accept_all_last_scale};
    F2cOptions options;
    options.line_mode = line_mode, options.subgrid = subgrid, options.derivative_weight = derivative_weight;
    options.level_dilation = level_dilation, options.dilation_kind = dilation_kind;
    options.equalize_mode = equalize_mode, options.equalize_ref_view = equalize_ref_view, options.equalize_joint = equalize_joint;
    options.equalize_max_gain = equalize_max_gain;
    return fine_to_coarse_one_context(ctx, req, options, {h_out_map_svu, h_out_valid_svu, n_levels, levels_out}, stats, nullptr);
}
RSLF_API_CATCH
