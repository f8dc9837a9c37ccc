// librslf_hip.so: the peak planes of a fine-to-coarse pyramid (include/rslf_hip.h, "peaks per level and validity by
// uniqueness") -- the two device-pointer primitives the level loop of rslf_f2c.hip calls for a kept run in the mode, beside
// rslf_f2c_tighten_bounds and rslf_f2c_fuse: the uniqueness predicate on a level's validity, and the fused peaks
// (k11_f2c_peaks.hpp).  Enqueued on the context's stream, not awaited.  One device.
#include "rslf_internal.hpp"
#include "rslf_plan_f2c_peaks.hpp"

#include <algorithm>

#include "k11_f2c_peaks.hpp"

using namespace rslf;

static_assert(kF2cPeakLevels == RSLF_F2C_MAX_LEVELS, "FusePeaksArgs holds one entry per level of the deepest pyramid");

extern "C" int rslf_f2c_unique_mask(rslf_ctx* ctx, uint8_t* d_valid, const rslf_peaks* d_pk, float ratio, size_t n) RSLF_API_TRY
{
    if (!ctx || !d_valid || !d_pk)
        return fail(RSLF_ERR_INVALID_ARG, "rslf_f2c_unique_mask: ctx, d_valid or d_pk is NULL");
    if (!d_pk->idx || !d_pk->score || !d_pk->runner_idx || !d_pk->runner_score)
        return fail(RSLF_ERR_INVALID_ARG, "rslf_f2c_unique_mask: d_pk needs idx, score, runner_idx and runner_score");
    if (!plan::f2c_uniqueness_ok(ratio) || ratio == 0.0f)
        return fail(RSLF_ERR_INVALID_ARG, "ratio=%g: the uniqueness ratio lies in (0, 1]", (double)ratio);
    if (n == 0)
        return RSLF_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(k11_unique_mask, dim3(blocks), dim3(256), 0, ctx->stream, d_valid, d_pk->idx, d_pk->score, d_pk->runner_idx,
                       d_pk->runner_score, ratio, (long long)n);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;   // enqueued, not awaited
}
RSLF_API_CATCH

extern "C" int rslf_f2c_fuse_peaks(rslf_ctx* ctx, const uint8_t* const* d_valid, const rslf_peaks* d_pk, const int* Vp, const int* Up,
                                   int P, int S, const rslf_peaks* d_out_svu, uint8_t* d_out_level_svu) RSLF_API_TRY
{
    if (!ctx || !d_valid || !d_pk || !Vp || !Up || !d_out_svu)
        return fail(RSLF_ERR_INVALID_ARG, "rslf_f2c_fuse_peaks: NULL argument");
    if (P < 1 || P > RSLF_F2C_MAX_LEVELS)
        return fail(RSLF_ERR_INVALID_ARG, "P=%d: a pyramid has 1 to %d levels", P, RSLF_F2C_MAX_LEVELS);
    if (S < 1)
        return fail(RSLF_ERR_INVALID_ARG, "S=%d", S);
    if (!d_out_svu->idx && !d_out_svu->score && !d_out_svu->runner_idx && !d_out_svu->runner_score && !d_out_level_svu)
        return fail(RSLF_ERR_INVALID_ARG, "rslf_f2c_fuse_peaks: every output plane is NULL, nothing to compute");
    FusePeaksArgs a = {};
    for (int p = 0; p < P; p++) {
        if (Vp[p] < 1 || Up[p] < 1)
            return fail(RSLF_ERR_INVALID_ARG, "level %d is %d x %d", p, Vp[p], Up[p]);
        if (!d_valid[p] || !d_pk[p].idx || !d_pk[p].score || !d_pk[p].runner_idx || !d_pk[p].runner_score)
            return fail(RSLF_ERR_INVALID_ARG, "level %d: d_valid and the four planes of d_pk must be given", p);
        if ((long long)S * Vp[p] * Up[p] <= 0)
            return fail(RSLF_ERR_INVALID_ARG, "level %d: S x V x U overflows", p);
        a.valid[p] = d_valid[p];
        a.idx[p] = d_pk[p].idx;
        a.score[p] = d_pk[p].score;
        a.runner_idx[p] = d_pk[p].runner_idx;
        a.runner_score[p] = d_pk[p].runner_score;
        a.V[p] = Vp[p];
        a.U[p] = Up[p];
        if (p > 0) {
            a.scale_v[p - 1] = f2c_walk_scale(Vp[p - 1], Vp[p]);
            a.scale_u[p - 1] = f2c_walk_scale(Up[p - 1], Up[p]);
        }
    }
    if (!plan::f2c_fuse_peaks_grid_ok(S, Vp[0], Up[0]))
        return fail(RSLF_ERR_UNSUPPORTED, "S=%d, V=%d: more views or scanlines than one launch's grid takes", S, Vp[0]);
    a.P = P;
    a.S = S;
    a.out_idx = d_out_svu->idx;
    a.out_score = d_out_svu->score;
    a.out_runner_idx = d_out_svu->runner_idx;
    a.out_runner_score = d_out_svu->runner_score;
    a.out_level = d_out_level_svu;
    HIP_TRY(hipSetDevice(ctx->device));
    const dim3 grid((unsigned)((Up[0] + plan::kFusePeaksBlock - 1) / plan::kFusePeaksBlock), (unsigned)Vp[0], (unsigned)S);
    hipLaunchKernelGGL(k11_fuse_peaks, grid, dim3(plan::kFusePeaksBlock), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;   // enqueued, not awaited
}
RSLF_API_CATCH
