// K6, the renderers: colour-mapped disparity maps and coloured EPIs (include/rslf_hip.h, "rendering").  The kernels are
// k6_render.hpp; every host-side decision is plan:: (rslf_plan.hpp, rslf_plan_render.hpp).  Scratch comes from the
// context's shared buffers (SharedBuf in rslf_internal.hpp: kSharedTable, the colour table and the per-plane render constants;
// kSharedLeft, the select states and the fits' results; kSharedRight, the slab of partial sums; the host-pointer forms stage
// in kSharedStagePlanes / Mask / Out), grow-only: a second call of the same size allocates nothing.
#include "rslf_internal.hpp"

#include "k6_render.hpp"

using namespace rslf;

namespace {

// The colour table, and behind it the (a, b) of every plane when h_minmax [n_planes][2] is given.
int upload_table(rslf_ctx* ctx, const uint8_t* lut_bgr, const uint8_t** d_lut, const double* h_minmax = nullptr, int n_planes = 0,
                 int affine = 0, const float2** d_ab = nullptr)
{
    void* p = nullptr;
    int rc = helper_scratch(ctx, kSharedTable, plan::render_table_bytes(n_planes), &p);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpyAsync(p, lut_bgr, plan::kRenderTableBytes, hipMemcpyHostToDevice, ctx->stream));
    *d_lut = (const uint8_t*)p;
    if (h_minmax) {
        std::vector<float> ab(2 * (size_t)n_planes);
        for (int k = 0; k < n_planes; k++) {
            const plan::RenderConsts c = plan::render_consts(affine, h_minmax[2 * k], h_minmax[2 * k + 1]);
            ab[2 * k] = c.a;
            ab[2 * k + 1] = c.b;
        }
        void* q = (char*)p + plan::kRenderTableBytes;
        HIP_TRY(hipMemcpyAsync(q, ab.data(), ab.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));   // pageable: staged before it returns
        *d_ab = (const float2*)q;
    }
    return RSLF_OK;
}

template <int C>
int launch_planes(hipStream_t st, dim3 grid, bool vec, const RenderArgs& A)
{
    if (vec)
        hipLaunchKernelGGL((k6_render_planes<C, true>), grid, dim3(plan::kRenderBlock), 0, st, A);
    else
        hipLaunchKernelGGL((k6_render_planes<C, false>), grid, dim3(plan::kRenderBlock), 0, st, A);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

bool fit_mode_ok(int mode)
{
    return mode == RSLF_FIT_MINMAX || mode == RSLF_FIT_QUANTILE || mode == RSLF_FIT_MEANSTD;
}

// The fit of n_planes planes: plan::fit_launches(mode) launches, one copy, one wait, whatever n_planes is.  The single
// call is the batch of one.  Arguments checked by the callers.
int fit_many(rslf_ctx* ctx, const float* d_planes, int n_planes, size_t plane_stride, int rows, int cols, size_t row_stride,
             const uint8_t* d_valid, int mode, double* h_minmax)
{
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int n = rows * cols;
    PlaneView pv;
    pv.p = d_planes;
    pv.valid = d_valid;
    pv.rows = rows;
    pv.cols = cols;
    pv.row_stride = (long long)row_stride;
    pv.plane_stride = n_planes > 1 ? (long long)plane_stride : 0;
    pv.vec = plan::fit_vec4_ok(cols, pv.row_stride, pv.plane_stride, n_planes, d_planes, d_valid) ? 1 : 0;
    void *state_p = nullptr, *slab_p = nullptr;
    int rc = helper_scratch(ctx, kSharedLeft, plan::fit_state_bytes(n_planes), &state_p);
    if (!rc)
        rc = helper_scratch(ctx, kSharedRight, plan::fit_slab_bytes(n_planes, n), &slab_p);
    if (rc)
        return rc;
    void* result_p = (char*)state_p + plan::fit_result_offset(n_planes);
    const int blocks = plan::fit_blocks(n);
    const dim3 grid((unsigned)plan::fit_batch_groups(n_planes, n), (unsigned)n_planes), per_plane((unsigned)n_planes);
    if (mode == RSLF_FIT_QUANTILE) {
        SelectState* state = (SelectState*)state_p;
        hipLaunchKernelGGL(k6_select_init, per_plane, dim3(plan::kRadixBins), 0, st, state, (uint32_t)plan::quantile_index(0.02, n),
                           (uint32_t)plan::quantile_index(0.98, n));
        HIP_TRY(hipGetLastError());
        for (int pass = 0; pass < plan::kRadixPasses; pass++) {
            hipLaunchKernelGGL(k6_select_count, grid, dim3(plan::kFitBlock), 0, st, pv, n, pass, state);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k6_select_narrow, per_plane, dim3(plan::kRadixBins), 0, st, state, pass, (float*)result_p);
            HIP_TRY(hipGetLastError());
        }
        std::vector<float> out(2 * (size_t)n_planes);
        HIP_TRY(hipMemcpyAsync(out.data(), result_p, out.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t i = 0; i < out.size(); i++)
            h_minmax[i] = out[i];
        return RSLF_OK;
    }
    hipLaunchKernelGGL(k6_fit_stats, grid, dim3(plan::kFitBlock), 0, st, pv, n, blocks, (FitPartial*)slab_p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k6_fit_reduce, per_plane, dim3(plan::kFitBlock), 0, st, (const FitPartial*)slab_p, blocks, (FitPartial*)result_p);
    HIP_TRY(hipGetLastError());
    std::vector<FitPartial> h((size_t)n_planes);
    HIP_TRY(hipMemcpyAsync(h.data(), result_p, h.size() * sizeof(FitPartial), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < n_planes; k++) {
        h_minmax[2 * k] = h[k].mn;
        h_minmax[2 * k + 1] = mode == RSLF_FIT_MINMAX ? (double)h[k].mx : plan::meanstd_max(h[k].sum, h[k].sumsq, n, h[k].mx);
    }
    return RSLF_OK;
}

int check_fit_args(const void* ctx, const void* planes, const void* out, int n_planes, int rows, int cols, size_t row_stride, int mode)
{
    if (!ctx || !planes || !out || n_planes < 1 || n_planes > plan::kRenderMaxPlanes || rows < 1 || cols < 1 || row_stride < (size_t)cols ||
        !fit_mode_ok(mode))
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    if ((long long)rows * cols > plan::kFitMaxPixels)
        return fail(RSLF_ERR_UNSUPPORTED, "a plane of %d x %d pixels is more than the fit counts in 32 bits", rows, cols);
    return RSLF_OK;
}

// rslf_render_planes (one range: h_minmax = {min, max}, each = false) and rslf_render_planes_each (h_minmax
// [n_planes][2]; an EPI batch may hold several scanlines).  Enqueued, not awaited.
int render_planes(rslf_ctx* ctx, const float* d_planes, int n_planes, size_t plane_stride, int rows, int cols, size_t row_stride,
                  const double* h_minmax, bool each, int formula, const uint8_t* lut_bgr, const uint8_t* d_valid, int mask_mode,
                  const rslf_volume* vol, int slice_kind, int index, float shadow_level, uint8_t* d_bgr_out)
{
    if (!ctx || !d_planes || !lut_bgr || !d_bgr_out || !h_minmax || n_planes < 1 || n_planes > plan::kRenderMaxPlanes || rows < 1 || cols < 1 ||
        row_stride < (size_t)cols || (formula != RSLF_RENDER_SHIFT && formula != RSLF_RENDER_AFFINE) ||
        (mask_mode != RSLF_MASK_BLACK && mask_mode != RSLF_MASK_ZERO_VALUE))
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    if (vol) {
        if (!vol->filled || vol->ctx != ctx)
            return fail(RSLF_ERR_INVALID_ARG, "the shadow cut's volume is empty or belongs to another context");
        if (vol->C != 1 && vol->C != 3)
            return fail(RSLF_ERR_UNSUPPORTED, "the shadow cut takes 1 or 3 channels, not %d", vol->C);
        if (slice_kind == RSLF_SLICE_VIEW) {
            if (rows != vol->V || cols != vol->U || index < 0 || index + n_planes > vol->S)
                return fail(RSLF_ERR_INVALID_ARG, "planes %d..%d of %d x %d do not lie in the volume's %d views of %d x %d", index,
                            index + n_planes - 1, rows, cols, vol->S, vol->V, vol->U);
        } else if (slice_kind == RSLF_SLICE_EPI) {
            if (!each && (n_planes != 1 || rows != vol->S || cols != vol->U || index < 0 || index >= vol->V))
                return fail(RSLF_ERR_INVALID_ARG, "an EPI slice is one %d x %d plane at a scanline below %d (got %d planes of %d x %d at %d)",
                            vol->S, vol->U, vol->V, n_planes, rows, cols, index);
            if (each && (rows != vol->S || cols != vol->U || index < 0 || index + n_planes > vol->V))
                return fail(RSLF_ERR_INVALID_ARG, "EPI slices %d..%d of %d x %d do not lie in the volume's %d scanlines of %d x %d", index,
                            index + n_planes - 1, rows, cols, vol->V, vol->S, vol->U);
        } else {
            return fail(RSLF_ERR_INVALID_ARG, "bad slice kind %d", slice_kind);
        }
    }
    HIP_TRY(hipSetDevice(ctx->device));
    RenderArgs A;
    memset(&A, 0, sizeof(A));
    const int affine = formula == RSLF_RENDER_AFFINE;
    int rc = each ? upload_table(ctx, lut_bgr, &A.lut_bgr, h_minmax, n_planes, affine, &A.ab) : upload_table(ctx, lut_bgr, &A.lut_bgr);
    if (rc)
        return rc;
    const plan::RenderConsts k = plan::render_consts(affine, h_minmax[0], h_minmax[1]);
    A.planes = d_planes;
    A.valid = d_valid;
    A.out = d_bgr_out;
    A.plane_stride = (long long)plane_stride;
    A.row_stride = (long long)row_stride;
    A.rows = rows;
    A.cols = cols;
    A.quads_per_row = (cols + 3) / 4;
    A.a = k.a;
    A.b = k.b;
    A.affine = affine;
    A.zero_value = mask_mode == RSLF_MASK_ZERO_VALUE;
    A.slice_epi = slice_kind == RSLF_SLICE_EPI;
    A.index = index;
    A.shadow_level = shadow_level;
    if (vol)
        A.vol = view_of(vol);
    const bool vec = plan::render_vec4_ok(cols, A.row_stride, n_planes > 1 ? A.plane_stride : 0, d_planes, d_valid, d_bgr_out);
    const long long quads = plan::render_quads(rows, cols);
    const dim3 grid((unsigned)((quads + plan::kRenderBlock - 1) / plan::kRenderBlock), (unsigned)n_planes);
    if (!vol)
        return launch_planes<0>(ctx->stream, grid, vec, A);
    return vol->C == 1 ? launch_planes<1>(ctx->stream, grid, vec, A) : launch_planes<3>(ctx->stream, grid, vec, A);
}

int epi_lines(rslf_ctx* ctx, const float* d_depth_vu, const uint8_t* d_mask_vu, int S, int U, int s_hat, int v_first, int n_rows,
              const uint8_t* lut_bgr, uint8_t* d_bgr_out)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t* d_lut = nullptr;
    int rc = upload_table(ctx, lut_bgr, &d_lut);
    if (rc)
        return rc;
    const int vec = (U % 4 == 0 && (uintptr_t)d_bgr_out % 4 == 0) ? 1 : 0;
    hipLaunchKernelGGL(k6_epi_lines, dim3((unsigned)S, (unsigned)n_rows), dim3(plan::kEpiLinesBlock), plan::epi_lines_lds_bytes(U), ctx->stream,
                       d_depth_vu, d_mask_vu, U, s_hat, v_first, d_lut, d_bgr_out, vec);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

int check_epi_lines_args(const void* ctx, const void* depth, const void* mask, const void* lut, const void* out, int V, int S, int U, int v_first,
                         int n_rows)
{
    if (!ctx || !depth || !mask || !lut || !out || V < 1 || S < 1 || U < 1 || v_first < 0 || n_rows < 1 || n_rows > 65535 ||
        v_first > V - n_rows)
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    if (U > plan::kEpiLinesMaxU)
        return fail(RSLF_ERR_UNSUPPORTED, "rows of %d columns: the line painter's z-buffer holds %d", U, plan::kEpiLinesMaxU);
    return RSLF_OK;
}

}  // namespace

extern "C" int rslf_render_centre_index(int n, int* index) RSLF_API_TRY
{
    if (!index)
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    *index = plan::centre_plane_index(n);
    if (*index < 0)
        return fail(RSLF_ERR_INVALID_ARG, "(int)std::round(%d / 2.0) is not below %d: the reference reads past its last plane here", n, n);
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_render_scaled_row(int v, int dim_v, int dim_v_orig, int* row) RSLF_API_TRY
{
    if (!row)
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    *row = plan::scaled_row_index(v, dim_v, dim_v_orig);
    if (*row < 0)
        return fail(RSLF_ERR_INVALID_ARG,
                    "scanline %d of %d has no row among the %d of this level: (int)std::round(1.0 * v * dim_v / dim_v_orig) is not "
                    "below dim_v (the reference reads past its last row here), or v is out of range", v, dim_v_orig, dim_v);
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_render_fit(rslf_ctx* ctx, const float* d_plane, int rows, int cols, size_t row_stride, const uint8_t* d_valid, int mode,
                               double* h_min, double* h_max) RSLF_API_TRY
{
    if (!h_min || !h_max)
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    int rc = check_fit_args(ctx, d_plane, h_min, 1, rows, cols, row_stride, mode);
    if (rc)
        return rc;
    double mm[2];
    rc = fit_many(ctx, d_plane, 1, 0, rows, cols, row_stride, d_valid, mode, mm);
    if (rc)
        return rc;
    *h_min = mm[0];
    *h_max = mm[1];
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_render_fit_many(rslf_ctx* ctx, const float* d_planes, int n_planes, size_t plane_stride, int rows, int cols, size_t row_stride,
                                    const uint8_t* d_valid, int mode, double* h_minmax) RSLF_API_TRY
{
    int rc = check_fit_args(ctx, d_planes, h_minmax, n_planes, rows, cols, row_stride, mode);
    if (rc)
        return rc;
    return fit_many(ctx, d_planes, n_planes, plane_stride, rows, cols, row_stride, d_valid, mode, h_minmax);
}
RSLF_API_CATCH

extern "C" int rslf_render_planes(rslf_ctx* ctx, const float* d_planes, int n_planes, size_t plane_stride, int rows, int cols, size_t row_stride,
                                  double min, double max, int formula, const uint8_t* lut_bgr, const uint8_t* d_valid, int mask_mode,
                                  const rslf_volume* vol, int slice_kind, int index, float shadow_level, uint8_t* d_bgr_out) RSLF_API_TRY
{
    const double mm[2] = {min, max};
    return render_planes(ctx, d_planes, n_planes, plane_stride, rows, cols, row_stride, mm, false, formula, lut_bgr, d_valid, mask_mode, vol,
                         slice_kind, index, shadow_level, d_bgr_out);   // enqueued, not awaited
}
RSLF_API_CATCH

extern "C" int rslf_render_planes_each(rslf_ctx* ctx, const float* d_planes, int n_planes, size_t plane_stride, int rows, int cols,
                                       size_t row_stride, const double* h_minmax, int formula, const uint8_t* lut_bgr, const uint8_t* d_valid,
                                       int mask_mode, const rslf_volume* vol, int slice_kind, int index, float shadow_level,
                                       uint8_t* d_bgr_out) RSLF_API_TRY
{
    return render_planes(ctx, d_planes, n_planes, plane_stride, rows, cols, row_stride, h_minmax, true, formula, lut_bgr, d_valid, mask_mode, vol,
                         slice_kind, index, shadow_level, d_bgr_out);   // enqueued, not awaited
}
RSLF_API_CATCH

extern "C" int rslf_render_epi_lines(rslf_ctx* ctx, const float* d_depth_vu, const uint8_t* d_mask_vu, int V, int S, int U, int s_hat, int v_first,
                                     int n_rows, const uint8_t* lut_bgr, uint8_t* d_bgr_out) RSLF_API_TRY
{
    int rc = check_epi_lines_args(ctx, d_depth_vu, d_mask_vu, lut_bgr, d_bgr_out, V, S, U, v_first, n_rows);
    if (rc)
        return rc;
    return epi_lines(ctx, d_depth_vu, d_mask_vu, S, U, s_hat, v_first, n_rows, lut_bgr, d_bgr_out);   // enqueued, not awaited
}
RSLF_API_CATCH

// ---- host-pointer forms: upload, the entries above, download, wait ---------------------------------------------------------

extern "C" int rslf_render_planes_host(rslf_ctx* ctx, const float* h_planes, int n_planes, size_t plane_stride, int rows, int cols,
                                       size_t row_stride, const uint8_t* h_valid, int fit_mode, int fit_plane, int fit_masked, int formula,
                                       const uint8_t* lut_bgr, int mask_mode, const rslf_volume* vol, int slice_kind, int index,
                                       float shadow_level, uint8_t* h_bgr_out, double* h_minmax) RSLF_API_TRY
{
    const bool given = fit_mode == RSLF_FIT_GIVEN;   // no fit: the ranges come in through h_minmax
    int rc = check_fit_args(ctx, h_planes, h_bgr_out, n_planes, rows, cols, row_stride, given ? RSLF_FIT_MINMAX : fit_mode);
    if (rc)
        return rc;
    if (given && !h_minmax)
        return fail(RSLF_ERR_INVALID_ARG, "RSLF_FIT_GIVEN needs h_minmax");
    if (!lut_bgr || fit_plane < -1 || fit_plane >= n_planes || (fit_masked && !h_valid) || (n_planes > 1 && plane_stride == 0))
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t extent = plan::planes_extent(n_planes, plane_stride, rows, cols, row_stride);
    const size_t out_bytes = (size_t)n_planes * rows * cols * 3;
    void *d_planes = nullptr, *d_valid = nullptr, *d_out = nullptr;
    rc = helper_scratch(ctx, kSharedStagePlanes, extent * sizeof(float), &d_planes);
    if (!rc && h_valid)
        rc = helper_scratch(ctx, kSharedStageMask, extent, &d_valid);
    if (!rc)
        rc = helper_scratch(ctx, kSharedStageOut, out_bytes, &d_out);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpyAsync(d_planes, h_planes, extent * sizeof(float), hipMemcpyHostToDevice, st));
    if (h_valid)
        HIP_TRY(hipMemcpyAsync(d_valid, h_valid, extent, hipMemcpyHostToDevice, st));
    const float* planes = (const float*)d_planes;
    const uint8_t* valid = (const uint8_t*)d_valid;
    std::vector<double> mm(2 * (size_t)n_planes);
    if (given) {
        std::copy(h_minmax, h_minmax + mm.size(), mm.begin());
    } else if (fit_plane < 0) {   // every plane through its own range
        rc = fit_many(ctx, planes, n_planes, plane_stride, rows, cols, row_stride, fit_masked ? valid : nullptr, fit_mode, mm.data());
    } else {               // every plane through plane fit_plane's range
        const size_t o = (size_t)fit_plane * plane_stride;
        rc = fit_many(ctx, planes + o, 1, 0, rows, cols, row_stride, fit_masked ? valid + o : nullptr, fit_mode, mm.data());
        for (int k = 1; k < n_planes; k++)
            mm[2 * k] = mm[0], mm[2 * k + 1] = mm[1];
    }
    if (!rc)
        rc = render_planes(ctx, planes, n_planes, plane_stride, rows, cols, row_stride, mm.data(), given || fit_plane < 0, formula, lut_bgr, valid, mask_mode,
                           vol, slice_kind, index, shadow_level, (uint8_t*)d_out);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpyAsync(h_bgr_out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_minmax && !given)
        std::copy(mm.begin(), mm.end(), h_minmax);
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_render_epi_lines_host(rslf_ctx* ctx, const float* h_depth_vu, const uint8_t* h_mask_vu, int V, int S, int U, int s_hat,
                                          int v_first, int n_rows, const uint8_t* lut_bgr, uint8_t* h_bgr_out) RSLF_API_TRY
{
    int rc = check_epi_lines_args(ctx, h_depth_vu, h_mask_vu, lut_bgr, h_bgr_out, V, S, U, v_first, n_rows);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)n_rows * U, out_bytes = (size_t)n_rows * S * U * 3;   // the scanlines asked for, no others
    void *d_depth = nullptr, *d_mask = nullptr, *d_out = nullptr;
    rc = helper_scratch(ctx, kSharedStagePlanes, n * sizeof(float), &d_depth);
    if (!rc)
        rc = helper_scratch(ctx, kSharedStageMask, n, &d_mask);
    if (!rc)
        rc = helper_scratch(ctx, kSharedStageOut, out_bytes, &d_out);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpyAsync(d_depth, h_depth_vu + (size_t)v_first * U, n * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_mask, h_mask_vu + (size_t)v_first * U, n, hipMemcpyHostToDevice, st));
    rc = epi_lines(ctx, (const float*)d_depth, (const uint8_t*)d_mask, S, U, s_hat, 0, n_rows, lut_bgr, (uint8_t*)d_out);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpyAsync(h_bgr_out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RSLF_OK;
}
RSLF_API_CATCH
