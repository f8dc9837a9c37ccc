// librslf_hip.so: cross-view consistency of a sweep's disparity planes (K12, k12_consistency.hpp) -- rslf_view_consistency on
// planes the caller holds on the device, rslf_view_consistency_host, which stages host planes through the context's shared
// buffers, and rslf_f2c_run_consistency (with its host-output form), which reads a kept fine-to-coarse run's planes in place.
// And its gate form (K13, k13_f2c_consistency.hpp): rslf_f2c_consistency_mask, the primitive the level loop of rslf_f2c.hip
// calls for a kept run with the gate set.  C-ABI: include/rslf_hip.h.  One device.
#include "rslf_internal.hpp"
#include "rslf_plan_f2c_consistency.hpp"

#include "k12_consistency.hpp"
#include "k13_f2c_consistency.hpp"

using namespace rslf;

namespace {

const rslf_view_counts kNoCounts = {nullptr, nullptr, nullptr, nullptr};

int count_planes(const rslf_view_counts& c) { return (c.seen != nullptr) + (c.agree != nullptr) + (c.above != nullptr) + (c.below != nullptr); }

// The argument checks every form shares (plan::consistency_args names the fault), then the grid's limits.
int check_consistency_args(const void* depth, const void* valid, int S, int V, int U, float tol, int min_agree, const rslf_view_counts& c,
                           const void* fused, const void* valid_out, unsigned* grid)
{
    if (!depth)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    const void* outs[6] = {c.seen, c.agree, c.above, c.below, fused, valid_out};
    bool any = false, aliased = false;
    for (const void* o : outs) {
        any = any || o != nullptr;
        aliased = aliased || (o != nullptr && (o == depth || o == valid));
    }
    switch (plan::consistency_args(S, V, U, tol, min_agree, any, aliased)) {
    case plan::kConsistencyOk:
        break;
    case plan::kConsistencyBadShape:
        return fail(RSLF_ERR_INVALID_ARG, "S=%d V=%d U=%d: not a stack of planes", S, V, U);
    case plan::kConsistencyBadTol:
        return fail(RSLF_ERR_INVALID_ARG, "tol=%g: a finite tolerance >= 0", (double)tol);
    case plan::kConsistencyBadMinAgree:
        return fail(RSLF_ERR_INVALID_ARG, "min_agree=%d: a count of views >= 0", min_agree);
    case plan::kConsistencyNoOutput:
        return fail(RSLF_ERR_INVALID_ARG, "all six output planes are NULL, nothing to compute");
    case plan::kConsistencyAlias:
        return fail(RSLF_ERR_INVALID_ARG, "an output plane is an input plane: the check reads the other views' rows while they are "
                                          "written (valid_out may not be the validity plane it reads)");
    }
    *grid = plan::consistency_grid(S, V, U);
    if (!*grid)
        return fail(RSLF_ERR_UNSUPPORTED, "S=%d V=%d U=%d exceed the grid limit of one launch (or U > %d)", S, V, U, plan::kConsistencyMaxU);
    return RSLF_OK;
}

// One launch on the context's stream; arguments checked.
int launch_consistency(rslf_ctx* ctx, unsigned grid, const float* depth, const uint8_t* valid, int S, int V, int U, float slope, float tol,
                       int radius, int min_agree, const rslf_view_counts& c, float* fused, uint8_t* valid_out)
{
    ConsistencyArgs a = {};
    a.depth = depth, a.valid = valid;
    a.S = S, a.V = V, a.U = U, a.nseg = plan::consistency_segments(U);
    a.slope = slope, a.tol = tol, a.radius = radius, a.min_agree = min_agree;
    a.order = ctx->consistency_order;
    a.seen = c.seen, a.agree = c.agree, a.above = c.above, a.below = c.below;
    a.fused = fused, a.valid_out = valid_out;
    if (valid)
        hipLaunchKernelGGL(k12_view_consistency<true>, dim3(grid), dim3(plan::kConsistencyBlock), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(k12_view_consistency<false>, dim3(grid), dim3(plan::kConsistencyBlock), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

// The launch on device inputs with the result planes on the HOST: the planes asked for are staged in the context's shared
// output buffer -- the 4-byte planes one after the other, the byte plane last --, copied out, and the stream awaited.
int consistency_to_host(rslf_ctx* ctx, unsigned grid, const float* d_depth, const uint8_t* d_valid, int S, int V, int U, float slope,
                        float tol, int radius, int min_agree, const rslf_view_counts& h, float* h_fused, uint8_t* h_valid_out)
{
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)S * V * U;
    void* d_stage = nullptr;
    int rc = helper_scratch(ctx, kSharedStageOut, n * plan::consistency_out_bytes_per_cell(count_planes(h), h_fused != nullptr, h_valid_out != nullptr),
                            &d_stage);
    if (rc)
        return rc;
    void* const host4[5] = {h.seen, h.agree, h.above, h.below, h_fused};
    void* dev4[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    char* at = static_cast<char*>(d_stage);
    for (int i = 0; i < 5; i++)
        if (host4[i]) {
            dev4[i] = at;
            at += n * 4;
        }
    uint8_t* const d_valid_out = h_valid_out ? reinterpret_cast<uint8_t*>(at) : nullptr;
    const rslf_view_counts dc = {static_cast<int32_t*>(dev4[0]), static_cast<int32_t*>(dev4[1]), static_cast<int32_t*>(dev4[2]),
                                 static_cast<int32_t*>(dev4[3])};
    rc = launch_consistency(ctx, grid, d_depth, d_valid, S, V, U, slope, tol, radius, min_agree, dc, static_cast<float*>(dev4[4]), d_valid_out);
    if (rc) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    for (int i = 0; i < 5; i++)
        if (host4[i])
            HIP_TRY(hipMemcpyAsync(host4[i], dev4[i], n * 4, hipMemcpyDeviceToHost, st));
    if (h_valid_out)
        HIP_TRY(hipMemcpyAsync(h_valid_out, d_valid_out, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RSLF_OK;
}

}  // namespace

extern "C" int rslf_view_consistency(rslf_ctx* ctx, const float* d_depth_svu, const uint8_t* d_valid_svu, int S, int V, int U, float slope,
                                     float tol, int radius, int min_agree, const rslf_view_counts* d_out, float* d_fused_svu,
                                     uint8_t* d_valid_out_svu) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    const rslf_view_counts& c = d_out ? *d_out : kNoCounts;
    unsigned grid = 0;
    int rc = check_consistency_args(d_depth_svu, d_valid_svu, S, V, U, tol, min_agree, c, d_fused_svu, d_valid_out_svu, &grid);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return launch_consistency(ctx, grid, d_depth_svu, d_valid_svu, S, V, U, slope, tol, radius, min_agree, c, d_fused_svu, d_valid_out_svu);
}
RSLF_API_CATCH

extern "C" int rslf_view_consistency_host(rslf_ctx* ctx, const float* h_depth_svu, const uint8_t* h_valid_svu, int S, int V, int U,
                                          float slope, float tol, int radius, int min_agree, const rslf_view_counts* h_out,
                                          float* h_fused_svu, uint8_t* h_valid_out_svu) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    const rslf_view_counts& c = h_out ? *h_out : kNoCounts;
    unsigned grid = 0;
    int rc = check_consistency_args(h_depth_svu, h_valid_svu, S, V, U, tol, min_agree, c, h_fused_svu, h_valid_out_svu, &grid);
    if (rc)
        return rc;
    if (ctx->sweep.open)
        return fail(RSLF_ERR_INVALID_ARG, "a sweep is open on this context");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)S * V * U;
    void *d_depth = nullptr, *d_valid = nullptr;
    rc = helper_scratch(ctx, kSharedStagePlanes, n * sizeof(float), &d_depth);
    if (!rc && h_valid_svu)
        rc = helper_scratch(ctx, kSharedStageMask, n, &d_valid);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpyAsync(d_depth, h_depth_svu, n * sizeof(float), hipMemcpyHostToDevice, st));
    if (h_valid_svu)
        HIP_TRY(hipMemcpyAsync(d_valid, h_valid_svu, n, hipMemcpyHostToDevice, st));
    return consistency_to_host(ctx, grid, static_cast<const float*>(d_depth), static_cast<const uint8_t*>(d_valid), S, V, U, slope, tol,
                               radius, min_agree, c, h_fused_svu, h_valid_out_svu);
}
RSLF_API_CATCH

// The gate form: the level's validity in, the gated validity out (another plane), the pixels made invalid added to *d_dropped.
extern "C" int rslf_f2c_consistency_mask(rslf_ctx* ctx, const float* d_depth_svu, const uint8_t* d_valid_svu, int S, int V, int U, float slope,
                                         float tol, int radius, int min_agree, uint8_t* d_valid_out_svu, int32_t* d_agree_svu,
                                         int32_t* d_seen_svu, unsigned long long* d_dropped) RSLF_API_TRY
{
    if (!ctx || !d_depth_svu || !d_valid_svu || !d_valid_out_svu)
        return fail(RSLF_ERR_INVALID_ARG, "rslf_f2c_consistency_mask: ctx, d_depth_svu, d_valid_svu or d_valid_out_svu is NULL");
    const void* outs[4] = {d_valid_out_svu, d_agree_svu, d_seen_svu, d_dropped};
    bool aliased = false;
    for (const void* o : outs)
        aliased = aliased || (o != nullptr && (o == (const void*)d_depth_svu || o == (const void*)d_valid_svu));
    switch (plan::f2c_consistency_mask_args(S, V, U, tol, min_agree, aliased)) {
    case plan::kConsistencyBadShape:
        return fail(RSLF_ERR_INVALID_ARG, "S=%d V=%d U=%d: not a stack of planes", S, V, U);
    case plan::kConsistencyBadTol:
        return fail(RSLF_ERR_INVALID_ARG, "tol=%g: a finite tolerance >= 0", (double)tol);
    case plan::kConsistencyBadMinAgree:
        return fail(RSLF_ERR_INVALID_ARG, "min_agree=%d: the gate asks for a count of agreeing views >= 1", min_agree);
    case plan::kConsistencyAlias:
        return fail(RSLF_ERR_INVALID_ARG, "an output plane is an input plane: the gate reads the other views' rows while they are "
                                          "written (d_valid_out_svu may not be the validity plane it reads)");
    default:
        break;
    }
    const unsigned grid = plan::consistency_grid(S, V, U);
    if (!grid)
        return fail(RSLF_ERR_UNSUPPORTED, "S=%d V=%d U=%d exceed the grid limit of one launch (or U > %d)", S, V, U, plan::kConsistencyMaxU);
    HIP_TRY(hipSetDevice(ctx->device));
    F2cConsistencyArgs a = {};
    a.depth = d_depth_svu, a.valid = d_valid_svu;
    a.S = S, a.V = V, a.U = U, a.nseg = plan::consistency_segments(U);
    a.slope = slope, a.tol = tol, a.radius = radius, a.min_agree = min_agree;
    a.order = ctx->consistency_order;
    a.valid_out = d_valid_out_svu, a.agree = d_agree_svu, a.seen = d_seen_svu, a.dropped = d_dropped;
    hipLaunchKernelGGL(k13_f2c_consistency_gate, dim3(grid), dim3(plan::kConsistencyBlock), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;   // enqueued, not awaited
}
RSLF_API_CATCH

// rslf_f2c_run_consistency and its host form: the kept planes are read in place
static int f2c_run_consistency(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, float tol, int radius, int min_agree,
                               const rslf_view_counts* out, float* fused_svu, uint8_t* valid_out_svu, bool host)
{
    if (!run || !ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (ctx->device != run->device)
        return fail(RSLF_ERR_INVALID_ARG, "the run lives on device %d, the context on device %d", run->device, ctx->device);
    if (level < 0 || level >= (int)run->kept.levels.size())
        return fail(RSLF_ERR_INVALID_ARG, "level %d of %d", level, (int)run->kept.levels.size());
    if (fused_result && level != 0)
        return fail(RSLF_ERR_INVALID_ARG, "the fused planes are at the finest size: ask for them with level 0, not %d", level);
    const F2cKeptLevel& kl = run->kept.levels[(size_t)level];
    const float* depth = fused_result ? run->kept.fused_map.as<const float>() : kl.depth.as<const float>();
    const uint8_t* valid = fused_result ? run->kept.fused_valid.as<const uint8_t>() : kl.valid.as<const uint8_t>();
    const rslf_view_counts& c = out ? *out : kNoCounts;
    unsigned grid = 0;
    int rc = check_consistency_args(depth, valid, run->S, kl.V, kl.U, tol, min_agree, c, fused_svu, valid_out_svu, &grid);
    if (rc)
        return rc;
    if (host && ctx->sweep.open)
        return fail(RSLF_ERR_INVALID_ARG, "a sweep is open on this context");
    HIP_TRY(hipSetDevice(ctx->device));
    // the slope factor the level's sweep propagated with (f2c.hpp:139); the fused planes are level 0's size: its factor
    if (host)
        return consistency_to_host(ctx, grid, depth, valid, run->S, kl.V, kl.U, kl.slope, tol, radius, min_agree, c, fused_svu, valid_out_svu);
    return launch_consistency(ctx, grid, depth, valid, run->S, kl.V, kl.U, kl.slope, tol, radius, min_agree, c, fused_svu, valid_out_svu);
}

extern "C" int rslf_f2c_run_consistency(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, float tol, int radius,
                                        int min_agree, const rslf_view_counts* d_out, float* d_fused_svu,
                                        uint8_t* d_valid_out_svu) RSLF_API_TRY
{
    return f2c_run_consistency(run, ctx, level, fused_result, tol, radius, min_agree, d_out, d_fused_svu, d_valid_out_svu, false);
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_consistency_host(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, float tol, int radius,
                                             int min_agree, const rslf_view_counts* h_out, float* h_fused_svu,
                                             uint8_t* h_valid_out_svu) RSLF_API_TRY
{
    return f2c_run_consistency(run, ctx, level, fused_result, tol, radius, min_agree, h_out, h_fused_svu, h_valid_out_svu, true);
}
RSLF_API_CATCH
