// librslf_hip.so: the scan's score matrix as an output (k2_scores.hpp) -- rslf_depth_epi_scores and its host form.
// C-ABI: include/rslf_hip.h.  One device; the streaming and on-chip kernels have no score form.
#include "rslf_internal.hpp"

#include <algorithm>

#include "k2_scores.hpp"

using namespace rslf;

static_assert(kScanWaves == plan::kScanWavesPerTile, "rslf_plan.hpp shares the hypotheses out over this many waves");

static int launch_score_rows_reg(int spad, int C, const ScanArgs& a, const ScoreDst& dst, dim3 grid, hipStream_t stream)
{
#define RSLF_CASE(N)                                                                                              \
    case N:                                                                                                       \
        hipLaunchKernelGGL((k2_score_rows_reg<N, RSLF_C>), grid, dim3(64 * kScanWaves), 0, stream, a, dst);       \
        return RSLF_OK;
    if (C == 1) {
        switch (spad) {
#define RSLF_C 1
            RSLF_SPAD_LIST_1CH(RSLF_CASE)
#undef RSLF_C
        default:
            break;
        }
    } else if (C == 3) {
        switch (spad) {
#define RSLF_C 3
            RSLF_SPAD_LIST_3CH(RSLF_CASE)
#undef RSLF_C
        default:
            break;
        }
    }
#undef RSLF_CASE
    return fail(RSLF_ERR_UNSUPPORTED, "no register score kernel with %d slots x %d channels", spad, C);
}

// Everything both forms check, before anything is queued (rslf_peaks.hip checks its windows the same way)
int rslf::check_score_args(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu, int dim_d, int s_hat,
                            const rslf_params* p, int v_first, int n_rows, const void* scores)
{
    if (!ctx || !vol || !scores)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    int rc = check_params(p);
    if (rc)
        return rc;
    if ((d_dmin_vu == nullptr) != (d_dmax_vu == nullptr))
        return fail(RSLF_ERR_INVALID_ARG, "d_dmin_vu and d_dmax_vu must both be given or both be NULL");
    if (dim_d < 2)
        return fail(RSLF_ERR_INVALID_ARG, "dim_d=%d: the hypothesis grid divides by dim_d-1 (core.hpp:548)", dim_d);
    if (s_hat < 0 || s_hat >= vol->S)
        return fail(RSLF_ERR_INVALID_ARG, "s_hat=%d outside [0,%d)", s_hat, vol->S);
    if (!vol->filled)
        return fail(RSLF_ERR_INVALID_ARG, "volume has not been filled");
    if (n_rows <= 0 || v_first < 0 || v_first >= vol->V || n_rows > vol->V - v_first)
        return fail(RSLF_ERR_INVALID_ARG, "scanlines [%d, %d + %d) are not a window of [0, %d)", v_first, v_first, n_rows, vol->V);
    if (ctx->sweep.open)
        return fail(RSLF_ERR_INVALID_ARG, "a sweep is open on this context: its pixel lists are in use");
    return RSLF_OK;
}

// The rows of scanlines [v_first, v_first + n_rows) into d_scores (that window's [n_rows][U][dim_d]); arguments checked.
int rslf::score_rows(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu, float dmin, float dmax,
                      int dim_d, int s_hat, const rslf_params* p, const uint8_t* d_mask_vu, int v_first, int n_rows, float* d_scores,
                      int* kind_out, int* spad_out, const ScoreLists* own)
{
    // (own lists: an open sweep's step -- the context's lists and pixel total are the sweep's, and already sized)
    int rc = own ? RSLF_OK : ensure_plane_scratch(ctx, vol->V, vol->U);
    if (rc)
        return rc;
    int spad = 0;
    const int kind = plan::choose_score_kernel(vol->S, vol->C, plan::scan_range_ok(vol->min_value, vol->max_value),
                                               p->interpolation == RSLF_INTERP_LINEAR, ctx->force_scan, &spad);
    const plan::ScanPlan sp = plan::score_plan(kind, spad, n_rows, vol->U, dim_d, ctx->num_cus, spad ? scan_reg_waves(spad, vol->C) : 4,
                                               ctx->force_groups);
    std::vector<plan::ScanLaunch> launches;
    long long tiles = 0;
    if (!plan::score_launches(v_first, n_rows, vol->U, sp, &launches, &tiles))
        return fail(RSLF_ERR_UNSUPPORTED, "%lld tiles x %d groups exceeds the grid limit", tiles, sp.groups);

    hipStream_t st = ctx->stream;
    const Scratch& sc = ctx->scratch;
    int* const list = own ? own->list : sc.list.as<int>();
    int* const count = own ? own->count : sc.count.as<int>();
    unsigned long long* const total = own ? own->total : sc.pixel_total();
    HIP_TRY(hipMemsetAsync(total, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_score_lists, dim3(n_rows), dim3(256), 0, st, d_mask_vu, vol->U, v_first, list, count, total);
    HIP_TRY(hipGetLastError());

    ScanArgs a = {};
    a.vol = view_of(vol);
    a.list = list;
    a.count = count;
    a.dmin_vu = d_dmin_vu;
    a.dmax_vu = d_dmax_vu;
    a.dmin = dmin;
    a.dmax = dmax;
    a.dim_d = dim_d;
    a.s_hat = s_hat;
    a.k = make_scan_consts(p);
    a.groups = sp.groups;
    a.tile_w = sp.tile_w;
    a.tiles_per_row = sp.tiles_per_row;
    a.tap_table = spad ? ctx->tap_table : 0;
    const ScoreDst dst = {d_scores, v_first};
    for (const plan::ScanLaunch& l : launches) {
        a.v0 = l.v0, a.logical_blocks = l.logical_blocks, a.per_xcd = l.per_xcd;
        // (dst.v_first stays the window's: a launch's rows are v0 .. within it)
        if (kind == RSLF_SCAN_REG) {
            rc = launch_score_rows_reg(spad, vol->C, a, dst, dim3(l.grid), st);
            if (rc)
                return rc;
        } else if (vol->C == 1) {
            hipLaunchKernelGGL(k2_score_rows_generic<1>, dim3(l.grid), dim3(64 * kScanWaves), 0, st, a, dst);
        } else {
            hipLaunchKernelGGL(k2_score_rows_generic<3>, dim3(l.grid), dim3(64 * kScanWaves), 0, st, a, dst);
        }
        HIP_TRY(hipGetLastError());
    }
    *kind_out = kind;
    *spad_out = spad;
    return RSLF_OK;
}

void rslf::score_stats(unsigned long long pixels, int dim_d, int kind, int spad, rslf_stats* stats)
{
    stats->pixels_scanned = (int64_t)pixels;
    stats->units = (int64_t)pixels * dim_d;
    stats->scan_kernel = kind;
    stats->s_pad = spad;
}

int rslf::read_pixel_total(rslf_ctx* ctx, unsigned long long* tot)
{
    HIP_TRY(hipMemcpyAsync(tot, ctx->scratch.pixel_total(), sizeof(*tot), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RSLF_OK;
}

extern "C" int rslf_depth_epi_scores(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu, float dmin,
                                     float dmax, int dim_d, int s_hat, const rslf_params* p, const uint8_t* d_mask_vu, int v_first,
                                     int n_rows, float* d_scores_vud, rslf_stats* stats) RSLF_API_TRY
{
    int rc = check_score_args(ctx, vol, d_dmin_vu, d_dmax_vu, dim_d, s_hat, p, v_first, n_rows, d_scores_vud);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    int kind = 0, spad = 0;
    rc = score_rows(ctx, vol, d_dmin_vu, d_dmax_vu, dmin, dmax, dim_d, s_hat, p, d_mask_vu, v_first, n_rows, d_scores_vud, &kind, &spad);
    if (rc || !stats)
        return rc;
    unsigned long long tot = 0;
    rc = read_pixel_total(ctx, &tot);   // (waits for the stream)
    if (rc == RSLF_OK)
        score_stats(tot, dim_d, kind, spad, stats);
    return rc;
}
RSLF_API_CATCH

extern "C" int rslf_depth_epi_scores_host(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu,
                                          float dmin, float dmax, int dim_d, int s_hat, const rslf_params* p, const uint8_t* h_mask_vu,
                                          int v_first, int n_rows, float* h_scores_vud, rslf_stats* stats) RSLF_API_TRY
{
    int rc = check_score_args(ctx, vol, d_dmin_vu, d_dmax_vu, dim_d, s_hat, p, v_first, n_rows, h_scores_vud);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    // the window in passes of as many scanlines as the staging budget holds (plan::kStagingBudget, or the "staging_kib" hook)
    const size_t budget = ctx->staging_kib > 0 ? (size_t)ctx->staging_kib << 10 : plan::kStagingBudget;
    const int pass_rows = std::min(n_rows, plan::score_window_rows(vol->U, dim_d, budget));
    const size_t row_floats = (size_t)vol->U * (size_t)dim_d;
    rc = ensure_staging(ctx, (size_t)pass_rows * row_floats * sizeof(float));
    if (rc)
        return rc;
    uint8_t* d_mask = nullptr;
    hipStream_t st = ctx->stream;
    if (h_mask_vu) {   // the window's rows of the mask, at their place in a [V][U] plane
        void* m = nullptr;
        rc = helper_scratch(ctx, kSharedStageMask, (size_t)vol->V * vol->U, &m);
        if (rc)
            return rc;
        d_mask = static_cast<uint8_t*>(m);
        const size_t first = (size_t)v_first * vol->U;
        HIP_TRY(hipMemcpyAsync(d_mask + first, h_mask_vu + first, (size_t)n_rows * vol->U, hipMemcpyHostToDevice, st));
    }
    float* const staging = ctx->scratch.staging.as<float>();
    unsigned long long pixels = 0;
    int kind = 0, spad = 0;
    for (int r0 = 0; r0 < n_rows; r0 += pass_rows) {
        const int rows = std::min(pass_rows, n_rows - r0);
        const size_t bytes = (size_t)rows * row_floats * sizeof(float);
        HIP_TRY(hipMemsetAsync(staging, 0, bytes, st));   // unscanned pixels: the reference's zero-filled buffer (core.hpp:167)
        rc = score_rows(ctx, vol, d_dmin_vu, d_dmax_vu, dmin, dmax, dim_d, s_hat, p, d_mask, v_first + r0, rows, staging, &kind, &spad);
        if (rc) {
            (void)hipStreamSynchronize(st);
            return rc;
        }
        HIP_TRY(hipMemcpyAsync(h_scores_vud + plan::score_offset(r0, 0, 0, vol->U, dim_d), staging, bytes, hipMemcpyDeviceToHost, st));
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
