// librslf_hip.so: the peaks mode of an open 2-D sweep (include/rslf_hip.h, rslf_sweep_peaks) -- the setter, and the step a
// visit queues after its scan (rslf_sweep.hip): over the visit's packed list with k10_peaks_list (k10_sweep_peaks.hpp), or
// window by window with the score rows (rslf_scores.hip's score_rows) and k8_score_peaks (rslf_peaks.hip), both untouched,
// on pixel lists of the step's own.  No score row is kept.  One device.
#include "rslf_internal.hpp"
#include "rslf_plan_subgrid.hpp"

#include <algorithm>

#include "k10_sweep_peaks.hpp"

using namespace rslf;

static size_t staging_budget(const rslf_ctx* ctx) { return ctx->staging_kib > 0 ? (size_t)ctx->staging_kib << 10 : plan::kStagingBudget; }

extern "C" int rslf_sweep_peaks(rslf_ctx* ctx, const rslf_volume* vol, const rslf_peaks* d_out_svu) RSLF_API_TRY
{
    if (!ctx || !vol)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    SweepState& sw = ctx->sweep;
    if (!sw.open || sw.scanned || !sw.first)
        return fail(RSLF_ERR_INVALID_ARG, "rslf_sweep_peaks belongs between rslf_sweep_begin and the first visit");
    if (d_out_svu && d_out_svu->disp)
        return fail(RSLF_ERR_INVALID_ARG, "rslf_sweep_peaks: disp must be NULL (the sub-grid mode puts that value in the depth plane)");
    if (d_out_svu && !d_out_svu->idx && !d_out_svu->score && !d_out_svu->runner_idx && !d_out_svu->runner_score)
        return fail(RSLF_ERR_INVALID_ARG, "rslf_sweep_peaks: all four planes are NULL, nothing to compute");
    if (d_out_svu && sw.dim_d > plan::kPeakMaxDimD)
        return fail(RSLF_ERR_INVALID_ARG, "dim_d=%d: the peaks take at most %d hypotheses", sw.dim_d, plan::kPeakMaxDimD);
    HIP_TRY(hipSetDevice(ctx->device));
    sw.peaks = false;
    sw.pk = rslf_peaks{};
    sw.prop_ratio = 0.0f;   // the gate by peak ratio reads these planes: every call here clears it (rslf_sweep_propagation_ratio follows)
    if (!d_out_svu)
        return RSLF_OK;
    // sized here, never inside a visit; held until rslf_sweep_end.  The visits' arg-max and score planes are the sub-grid
    // mode's (with line confidence on, the arg-max plane is K7's); the lists, counts and mask are this step's alone.
    Scratch& sc = ctx->scratch;
    const int V = vol->V, U = vol->U;
    const size_t plane = plan::sweep_subgrid_plane_bytes(true, V, U);
    if (sw.lc_mode == RSLF_LINE_CONF_OFF)
        HIP_TRY(hip_err(sc.sub_idx.reserve(plane)));
    HIP_TRY(hip_err(sc.sub_score.reserve(plane)));
    HIP_TRY(hip_err(sc.pk_list.reserve(plan::sweep_peaks_list_bytes(true, V, U))));
    HIP_TRY(hip_err(sc.pk_count.reserve(plan::sweep_peaks_count_bytes(true, V, U))));
    HIP_TRY(hip_err(sc.pk_mask.reserve(plan::sweep_peaks_mask_bytes(true, V, U))));
    int rc = ensure_staging(ctx, plan::sweep_peaks_staging_bytes(V, U, sw.dim_d, staging_budget(ctx)));
    if (rc)
        return rc;
    sw.pk = *d_out_svu;
    sw.peaks = true;
    return RSLF_OK;
}
RSLF_API_CATCH

// The list form: one launch, a wave per entry of Scratch::list / packed_len() as the visit's scan took them.
static int peaks_list(rslf_ctx* ctx, const ScanArgs& scan, const SweepPeaksArgs& q, int C)
{
    ScanArgs a = scan;
    a.list = ctx->scratch.list.as<int>();
    a.packed_n = ctx->scratch.packed_len();
    const dim3 grid(plan::peaks_list_blocks(a.vol.V, a.vol.U, ctx->num_cus)), block(64 * plan::kPeaksListWaves);
    hipStream_t st = ctx->stream;
    bool launched = false;
#define RSLF_K10_CASE(CC, MODE)                                                             \
    if (!launched && C == CC && a.k.interp == MODE) {                                       \
        hipLaunchKernelGGL((k10_peaks_list<CC, MODE>), grid, block, 0, st, a, q);           \
        launched = true;                                                                    \
    }
    RSLF_K10_CASE(1, 0)
    RSLF_K10_CASE(1, 1)
    RSLF_K10_CASE(1, 2)
    RSLF_K10_CASE(3, 0)
    RSLF_K10_CASE(3, 1)
    RSLF_K10_CASE(3, 2)
#undef RSLF_K10_CASE
    if (!launched)
        return fail(RSLF_ERR_INTERNAL, "no sweep-peaks kernel for %d channels, interpolation %d", C, a.k.interp);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

// The dense form: the mask "idx >= 0", then the plane window by window through the staging buffer -- the rows of a pass, then
// their peaks; a pass's score kernels run after the peaks of the one before have read the buffer (one stream).
static int peaks_dense(rslf_ctx* ctx, const rslf_volume* vol, const float* dmin_vu, const float* dmax_vu, float dmin, float dmax,
                       int dim_d, int s_hat, const rslf_params* p, const int32_t* idx_vu, const rslf_peaks& out_vu)
{
    const int V = vol->V, U = vol->U;
    const size_t n = (size_t)V * U;
    Scratch& sc = ctx->scratch;
    hipStream_t st = ctx->stream;
    const int pass_rows = plan::sweep_peaks_pass_rows(V, U, dim_d, staging_budget(ctx));
    // (already this large unless the visit's dim_d is not the one rslf_sweep_begin was given)
    int rc = ensure_staging(ctx, plan::peaks_staging_bytes(pass_rows, U, dim_d, false));
    if (rc)
        return rc;
    uint8_t* const mask = sc.pk_mask.as<uint8_t>();
    hipLaunchKernelGGL(k10_accepted_mask, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, idx_vu, mask, (long long)n);
    HIP_TRY(hipGetLastError());
    ScoreLists own;
    own.list = sc.pk_list.as<int>();
    own.count = sc.pk_count.as<int>();
    own.total = reinterpret_cast<unsigned long long*>(sc.pk_count.as<char>() + plan::sweep_peaks_count_offset_total(V));
    float* const rows_buf = sc.staging.as<float>();
    int kind = 0, spad = 0;
    for (int r0 = 0; r0 < V; r0 += pass_rows) {
        const int rows = std::min(pass_rows, V - r0);
        const size_t at = (size_t)r0 * U;
        rc = score_rows(ctx, vol, dmin_vu, dmax_vu, dmin, dmax, dim_d, s_hat, p, mask, r0, rows, rows_buf, &kind, &spad, &own);
        if (rc)
            return rc;
        rslf_peaks w = {};
        w.idx = out_vu.idx ? out_vu.idx + at : nullptr;
        w.score = out_vu.score ? out_vu.score + at : nullptr;
        w.runner_idx = out_vu.runner_idx ? out_vu.runner_idx + at : nullptr;
        w.runner_score = out_vu.runner_score ? out_vu.runner_score + at : nullptr;
        rc = launch_score_peaks(ctx, rows_buf, U, dim_d, dmin_vu, dmax_vu, dmin, dmax, mask, r0, rows, w);
        if (rc)
            return rc;
    }
    return RSLF_OK;
}

int rslf::sweep_peaks_step(rslf_ctx* ctx, const rslf_volume* vol, const float* dmin_vu, const float* dmax_vu, float dmin, float dmax,
                           int dim_d, int s_hat, const rslf_params* p, const int32_t* idx_vu, int form)
{
    if (form == plan::kPeaksNone)
        return RSLF_OK;
    const size_t at = (size_t)s_hat * vol->V * vol->U;
    const rslf_peaks& pk = ctx->sweep.pk;
    rslf_peaks out = {};
    out.idx = pk.idx ? pk.idx + at : nullptr;
    out.score = pk.score ? pk.score + at : nullptr;
    out.runner_idx = pk.runner_idx ? pk.runner_idx + at : nullptr;
    out.runner_score = pk.runner_score ? pk.runner_score + at : nullptr;
    if (form == plan::kPeaksDense)
        return peaks_dense(ctx, vol, dmin_vu, dmax_vu, dmin, dmax, dim_d, s_hat, p, idx_vu, out);
    if ((size_t)vol->V * vol->U > (size_t)INT32_MAX)
        return fail(RSLF_ERR_INTERNAL, "a plane of %d x %d pixels has no packed list", vol->V, vol->U);
    ScanArgs a = {};
    a.vol = view_of(vol);
    a.dmin_vu = dmin_vu;
    a.dmax_vu = dmax_vu;
    a.dmin = dmin;
    a.dmax = dmax;
    a.dim_d = dim_d;
    a.s_hat = s_hat;
    a.k = make_scan_consts(p);
    a.groups = 1;
    SweepPeaksArgs q = {};
    q.idx = idx_vu;
    q.out_idx = out.idx, q.out_score = out.score, q.out_runner_idx = out.runner_idx, q.out_runner_score = out.runner_score;
    return peaks_list(ctx, a, q, vol->C);
}
