// librslf_hip.so: the peaks of the score rows (k8_peaks.hpp) -- rslf_score_peaks on rows the caller holds, and
// rslf_depth_epi_peaks / rslf_depth_epi_peaks_host, which make the rows of a window pass by pass in the context's staging
// buffer (rslf_scores.hip's score_rows, untouched) and reduce them there: the rows never leave the device.
// C-ABI: include/rslf_hip.h.  One device.
#include "rslf_internal.hpp"

#include <algorithm>

#include "k8_peaks.hpp"

using namespace rslf;

static bool any_plane(const rslf_peaks* o) { return o->idx || o->score || o->disp || o->runner_idx || o->runner_score; }

// k8_score_peaks over the pixels of scanlines [v_first, v_first + n_rows) of [V][U] planes; arguments checked
int rslf::launch_score_peaks(rslf_ctx* ctx, const float* d_scores, int U, int dim_d, const float* d_dmin_vu, const float* d_dmax_vu,
                             float dmin, float dmax, const uint8_t* d_mask_vu, int v_first, int n_rows, const rslf_peaks& out)
{
    PeakArgs a = {};
    a.scores = d_scores;
    a.mask = d_mask_vu;
    a.dmin_vu = d_dmin_vu;
    a.dmax_vu = d_dmax_vu;
    a.dmin = dmin;
    a.dmax = dmax;
    a.first = (long long)v_first * U;
    a.n_pixels = (long long)n_rows * U;
    a.dim_d = dim_d;
    a.n_blocks = plan::peak_blocks(dim_d);
    a.idx = out.idx, a.score = out.score, a.disp = out.disp, a.runner_idx = out.runner_idx, a.runner_score = out.runner_score;
    const unsigned grid = plan::peaks_grid(a.n_pixels);
    if (!grid)
        return fail(RSLF_ERR_UNSUPPORTED, "%lld pixels exceed the grid limit", a.n_pixels);
    hipLaunchKernelGGL(k8_score_peaks, dim3(grid), dim3(64 * plan::kPeakWaves), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

static int check_peaks_out(const rslf_peaks* out, int dim_d)
{
    if (!out)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (!any_plane(out))
        return fail(RSLF_ERR_INVALID_ARG, "rslf_peaks: all five planes are NULL, nothing to compute");
    if (dim_d > plan::kPeakMaxDimD)
        return fail(RSLF_ERR_INVALID_ARG, "dim_d=%d: the peaks take at most %d hypotheses", dim_d, plan::kPeakMaxDimD);
    return RSLF_OK;
}

static size_t staging_budget(const rslf_ctx* ctx) { return ctx->staging_kib > 0 ? (size_t)ctx->staging_kib << 10 : plan::kStagingBudget; }

// the planes of `out` moved on by `px` pixels (a pass of a window)
static rslf_peaks planes_at(const rslf_peaks& o, size_t px)
{
    rslf_peaks q = o;
    q.idx = o.idx ? o.idx + px : nullptr;
    q.score = o.score ? o.score + px : nullptr;
    q.disp = o.disp ? o.disp + px : nullptr;
    q.runner_idx = o.runner_idx ? o.runner_idx + px : nullptr;
    q.runner_score = o.runner_score ? o.runner_score + px : nullptr;
    return q;
}

extern "C" int rslf_score_peaks(rslf_ctx* ctx, const float* d_scores_vud, int U, int dim_d, const float* d_dmin_vu, const float* d_dmax_vu,
                                float dmin, float dmax, const uint8_t* d_mask_vu, int v_first, int n_rows,
                                const rslf_peaks* d_out) RSLF_API_TRY
{
    if (!ctx || !d_scores_vud)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    int rc = check_peaks_out(d_out, dim_d);
    if (rc)
        return rc;
    if ((d_dmin_vu == nullptr) != (d_dmax_vu == nullptr))
        return fail(RSLF_ERR_INVALID_ARG, "d_dmin_vu and d_dmax_vu must both be given or both be NULL");
    if (dim_d < 2)
        return fail(RSLF_ERR_INVALID_ARG, "dim_d=%d: the hypothesis grid divides by dim_d-1", dim_d);
    if (U < 1 || n_rows <= 0 || v_first < 0)
        return fail(RSLF_ERR_INVALID_ARG, "U=%d, scanlines [%d, %d + %d): not a window of rows", U, v_first, v_first, n_rows);
    if (ctx->sweep.open)
        return fail(RSLF_ERR_INVALID_ARG, "a sweep is open on this context");
    HIP_TRY(hipSetDevice(ctx->device));
    return launch_score_peaks(ctx, d_scores_vud, U, dim_d, d_dmin_vu, d_dmax_vu, dmin, dmax, d_mask_vu, v_first, n_rows, *d_out);
}
RSLF_API_CATCH

extern "C" int rslf_depth_epi_peaks(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu, float dmin,
                                    float dmax, int dim_d, int s_hat, const rslf_params* p, const uint8_t* d_mask_vu, int v_first,
                                    int n_rows, const rslf_peaks* d_out, rslf_stats* stats) RSLF_API_TRY
{
    int rc = check_score_args(ctx, vol, d_dmin_vu, d_dmax_vu, dim_d, s_hat, p, v_first, n_rows, d_out);
    if (rc)
        return rc;
    rc = check_peaks_out(d_out, dim_d);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const int pass_rows = std::min(n_rows, plan::peaks_window_rows(vol->U, dim_d, staging_budget(ctx)));
    rc = ensure_staging(ctx, plan::peaks_staging_bytes(pass_rows, vol->U, dim_d, false));
    if (rc)
        return rc;
    float* const rows_buf = ctx->scratch.staging.as<float>();
    unsigned long long pixels = 0;
    int kind = 0, spad = 0;
    // pass after pass on the stream: a pass's score kernels run after the peaks of the one before have read the buffer
    for (int r0 = 0; r0 < n_rows; r0 += pass_rows) {
        const int rows = std::min(pass_rows, n_rows - r0);
        rc = score_rows(ctx, vol, d_dmin_vu, d_dmax_vu, dmin, dmax, dim_d, s_hat, p, d_mask_vu, v_first + r0, rows, rows_buf, &kind, &spad);
        if (rc == RSLF_OK)
            rc = launch_score_peaks(ctx, rows_buf, vol->U, dim_d, d_dmin_vu, d_dmax_vu, dmin, dmax, d_mask_vu, v_first + r0, rows,
                              planes_at(*d_out, (size_t)r0 * vol->U));
        if (rc)
            return rc;
        if (stats) {   // (waits: the total is zeroed by the next pass)
            unsigned long long tot = 0;
            rc = read_pixel_total(ctx, &tot);
            if (rc)
                return rc;
            pixels += tot;
        }
    }
    if (stats)
        score_stats(pixels, dim_d, kind, spad, stats);
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_depth_epi_peaks_host(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu,
                                         float dmin, float dmax, int dim_d, int s_hat, const rslf_params* p, const uint8_t* h_mask_vu,
                                         int v_first, int n_rows, const rslf_peaks* h_out, rslf_stats* stats) RSLF_API_TRY
{
    int rc = check_score_args(ctx, vol, d_dmin_vu, d_dmax_vu, dim_d, s_hat, p, v_first, n_rows, h_out);
    if (rc)
        return rc;
    rc = check_peaks_out(h_out, dim_d);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const int pass_rows = std::min(n_rows, plan::peaks_window_rows(vol->U, dim_d, staging_budget(ctx)));
    rc = ensure_staging(ctx, plan::peaks_staging_bytes(pass_rows, vol->U, dim_d, true));
    if (rc)
        return rc;
    hipStream_t st = ctx->stream;
    uint8_t* d_mask = nullptr;
    if (h_mask_vu) {   // the window's rows of the mask, at their place in a [V][U] plane
        void* m = nullptr;
        rc = helper_scratch(ctx, kSharedStageMask, (size_t)vol->V * vol->U, &m);
        if (rc)
            return rc;
        d_mask = static_cast<uint8_t*>(m);
        const size_t first = (size_t)v_first * vol->U;
        HIP_TRY(hipMemcpyAsync(d_mask + first, h_mask_vu + first, (size_t)n_rows * vol->U, hipMemcpyHostToDevice, st));
    }
    // the staging buffer: a pass's rows, then its five planes -- the two index planes first, so that one fill gives them -1
    float* const rows_buf = ctx->scratch.staging.as<float>();
    const size_t pass_px = (size_t)pass_rows * vol->U;
    float* const planes = rows_buf + pass_px * (size_t)dim_d;
    rslf_peaks d = {};
    d.idx = reinterpret_cast<int32_t*>(planes);
    d.runner_idx = reinterpret_cast<int32_t*>(planes + pass_px);
    d.score = planes + 2 * pass_px;
    d.disp = planes + 3 * pass_px;
    d.runner_score = planes + 4 * pass_px;
    unsigned long long pixels = 0;
    int kind = 0, spad = 0;
    for (int r0 = 0; r0 < n_rows; r0 += pass_rows) {
        const int rows = std::min(pass_rows, n_rows - r0);
        const size_t px = (size_t)rows * vol->U, at = (size_t)r0 * vol->U;
        HIP_TRY(hipMemsetAsync(planes, 0xFF, 2 * pass_px * sizeof(float), st));       // unscanned pixels: no index ...
        HIP_TRY(hipMemsetAsync(planes + 2 * pass_px, 0, 3 * pass_px * sizeof(float), st));   // ... and 0
        rc = score_rows(ctx, vol, d_dmin_vu, d_dmax_vu, dmin, dmax, dim_d, s_hat, p, d_mask, v_first + r0, rows, rows_buf, &kind, &spad);
        if (rc == RSLF_OK)
            rc = launch_score_peaks(ctx, rows_buf, vol->U, dim_d, d_dmin_vu, d_dmax_vu, dmin, dmax, d_mask, v_first + r0, rows, d);
        if (rc) {
            (void)hipStreamSynchronize(st);
            return rc;
        }
        const struct { void* host; const void* dev; } copies[5] = {{h_out->idx ? h_out->idx + at : nullptr, d.idx},
                                                                    {h_out->score ? h_out->score + at : nullptr, d.score},
                                                                    {h_out->disp ? h_out->disp + at : nullptr, d.disp},
                                                                    {h_out->runner_idx ? h_out->runner_idx + at : nullptr, d.runner_idx},
                                                                    {h_out->runner_score ? h_out->runner_score + at : nullptr, d.runner_score}};
        for (const auto& c : copies)
            if (c.host)
                HIP_TRY(hipMemcpyAsync(c.host, c.dev, px * sizeof(float), hipMemcpyDeviceToHost, st));
        unsigned long long tot = 0;
        rc = read_pixel_total(ctx, &tot);   // waits: the staging buffer is reused by the next pass
        if (rc)
            return rc;
        pixels += tot;
    }
    if (stats)
        score_stats(pixels, dim_d, kind, spad, stats);
    return RSLF_OK;
}
RSLF_API_CATCH
