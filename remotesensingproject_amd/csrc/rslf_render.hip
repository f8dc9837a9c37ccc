// K6, the renderers: colour-mapped disparity maps and coloured EPIs (include/rslf_hip.h, "rendering").  The kernels are
// k6_render.hpp; every host-side decision is plan:: (rslf_plan.hpp).  Scratch comes from the context's helper slots
// (1: the table, 2: the select state and the reduced sums, 3: the slab of partial sums), grow-only: a second call
// allocates nothing.
#include "rslf_internal.hpp"

#include "k6_render.hpp"

using namespace rslf;

namespace {

constexpr size_t kFitResultOffset = (sizeof(SelectState) + 15) / 16 * 16;   // FitPartial behind the select state in slot 2

int upload_table(rslf_ctx* ctx, const uint8_t* lut_bgr, const uint8_t** d_lut)
{
    void* p = nullptr;
    int rc = helper_scratch(ctx, 1, 256 * 3, &p);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpyAsync(p, lut_bgr, 256 * 3, hipMemcpyHostToDevice, ctx->stream));
    *d_lut = (const uint8_t*)p;
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
    if (!ctx || !d_plane || !h_min || !h_max || rows < 1 || cols < 1 || row_stride < (size_t)cols ||
        (mode != RSLF_FIT_MINMAX && mode != RSLF_FIT_QUANTILE && mode != RSLF_FIT_MEANSTD))
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    if ((long long)rows * cols > (long long)1 << 30)
        return fail(RSLF_ERR_UNSUPPORTED, "a plane of %d x %d pixels is more than the fit counts in 32 bits", rows, cols);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int n = rows * cols;
    PlaneView pv;
    pv.p = d_plane;
    pv.valid = d_valid;
    pv.rows = rows;
    pv.cols = cols;
    pv.row_stride = (long long)row_stride;
    pv.vec = plan::render_vec4_ok(cols, (long long)row_stride, 0, d_plane, d_valid, nullptr) ? 1 : 0;
    void *state_p = nullptr, *slab_p = nullptr;
    int rc = helper_scratch(ctx, 2, kFitResultOffset + sizeof(FitPartial), &state_p);
    if (!rc)
        rc = helper_scratch(ctx, 3, (size_t)plan::kFitMaxBlocks * sizeof(FitPartial), &slab_p);
    if (rc)
        return rc;
    const int blocks = plan::fit_blocks(n);
    if (mode == RSLF_FIT_QUANTILE) {
        SelectState* state = (SelectState*)state_p;
        hipLaunchKernelGGL(k6_select_init, dim3(1), dim3(plan::kRadixBins), 0, st, state, (uint32_t)plan::quantile_index(0.02, n),
                           (uint32_t)plan::quantile_index(0.98, n));
        HIP_TRY(hipGetLastError());
        for (int pass = 0; pass < plan::kRadixPasses; pass++) {
            hipLaunchKernelGGL(k6_select_count, dim3(blocks), dim3(plan::kFitBlock), 0, st, pv, n, pass, state);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k6_select_narrow, dim3(1), dim3(plan::kRadixBins), 0, st, state, pass);
            HIP_TRY(hipGetLastError());
        }
        float out[2];
        HIP_TRY(hipMemcpyAsync(out, (const char*)state_p + offsetof(SelectState, out), sizeof(out), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        *h_min = out[0];
        *h_max = out[1];
        return RSLF_OK;
    }
    FitPartial* result = (FitPartial*)((char*)state_p + kFitResultOffset);
    hipLaunchKernelGGL(k6_fit_stats, dim3(blocks), dim3(plan::kFitBlock), 0, st, pv, n, (FitPartial*)slab_p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k6_fit_reduce, dim3(1), dim3(plan::kFitBlock), 0, st, (const FitPartial*)slab_p, blocks, result);
    HIP_TRY(hipGetLastError());
    FitPartial h;
    HIP_TRY(hipMemcpyAsync(&h, result, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *h_min = h.mn;
    *h_max = mode == RSLF_FIT_MINMAX ? (double)h.mx : plan::meanstd_max(h.sum, h.sumsq, n, h.mx);
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_render_planes(rslf_ctx* ctx, const float* d_planes, int n_planes, size_t plane_stride, int rows, int cols, size_t row_stride,
                                  double min, double max, int formula, const uint8_t* lut_bgr, const uint8_t* d_valid, int mask_mode,
                                  const rslf_volume* vol, int slice_kind, int index, float shadow_level, uint8_t* d_bgr_out) RSLF_API_TRY
{
    if (!ctx || !d_planes || !lut_bgr || !d_bgr_out || n_planes < 1 || n_planes > 65535 || rows < 1 || cols < 1 || row_stride < (size_t)cols ||
        (formula != RSLF_RENDER_SHIFT && formula != RSLF_RENDER_AFFINE) || (mask_mode != RSLF_MASK_BLACK && mask_mode != RSLF_MASK_ZERO_VALUE))
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
            if (n_planes != 1 || rows != vol->S || cols != vol->U || index < 0 || index >= vol->V)
                return fail(RSLF_ERR_INVALID_ARG, "an EPI slice is one %d x %d plane at a scanline below %d (got %d planes of %d x %d at %d)",
                            vol->S, vol->U, vol->V, n_planes, rows, cols, index);
        } else {
            return fail(RSLF_ERR_INVALID_ARG, "bad slice kind %d", slice_kind);
        }
    }
    HIP_TRY(hipSetDevice(ctx->device));
    RenderArgs A;
    memset(&A, 0, sizeof(A));
    int rc = upload_table(ctx, lut_bgr, &A.lut_bgr);
    if (rc)
        return rc;
    const plan::RenderConsts k = plan::render_consts(formula == RSLF_RENDER_AFFINE, min, max);
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
    A.affine = formula == RSLF_RENDER_AFFINE;
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
    return vol->C == 1 ? launch_planes<1>(ctx->stream, grid, vec, A) : launch_planes<3>(ctx->stream, grid, vec, A);   // enqueued, not awaited
}
RSLF_API_CATCH

extern "C" int rslf_render_epi_lines(rslf_ctx* ctx, const float* d_depth_vu, const uint8_t* d_mask_vu, int V, int S, int U, int s_hat, int v_first,
                                     int n_rows, const uint8_t* lut_bgr, uint8_t* d_bgr_out) RSLF_API_TRY
{
    if (!ctx || !d_depth_vu || !d_mask_vu || !lut_bgr || !d_bgr_out || V < 1 || S < 1 || U < 1 || v_first < 0 || n_rows < 1 ||
        n_rows > 65535 || v_first > V - n_rows)
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    if (U > plan::kEpiLinesMaxU)
        return fail(RSLF_ERR_UNSUPPORTED, "rows of %d columns: the line painter's z-buffer holds %d", U, plan::kEpiLinesMaxU);
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t* d_lut = nullptr;
    int rc = upload_table(ctx, lut_bgr, &d_lut);
    if (rc)
        return rc;
    const int vec = (U % 4 == 0 && (uintptr_t)d_bgr_out % 4 == 0) ? 1 : 0;
    hipLaunchKernelGGL(k6_epi_lines, dim3((unsigned)S, (unsigned)n_rows), dim3(plan::kEpiLinesBlock), plan::epi_lines_lds_bytes(U), ctx->stream,
                       d_depth_vu, d_mask_vu, U, s_hat, v_first, d_lut, d_bgr_out, vec);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;   // enqueued, not awaited
}
RSLF_API_CATCH
