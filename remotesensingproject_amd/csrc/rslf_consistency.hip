// librslf_hip.so: cross-view consistency of a sweep's disparity planes (K12, k12_consistency.hpp) -- rslf_view_consistency on
// planes the caller holds on the device, rslf_view_consistency_host, which stages host planes through the context's shared
// buffers, and rslf_f2c_run_consistency (with its host-output form), which reads a kept fine-to-coarse run's planes in place.
// And its gate form (K13, k13_f2c_consistency.hpp): rslf_f2c_consistency_mask, the primitive the level loop of rslf_f2c.hip
// calls for a kept run with the gate set.  C-ABI: include/rslf_hip.h.  One device.
#include "rslf_internal.hpp"
#include "rslf_plan_f2c_consistency.hpp"
#include "rslf_stack_op.hpp"

#include "k12_consistency.hpp"
#include "k13_f2c_consistency.hpp"

using namespace rslf;

namespace {

const rslf_view_counts kNoCounts = {nullptr, nullptr, nullptr, nullptr};

// What a call asks for besides its inputs.
struct Request {
    float tol;
    int radius, min_agree;
    const rslf_view_counts* counts;   // nullable: none of the four
    float* fused;
    uint8_t* valid_out;
};

// The argument checks every form shares (plan::consistency_args names the fault), then the grid's limits.
int check_consistency_args(const StackIn& in, const Request& r, unsigned* grid)
{
    const int S = in.S, V = in.V, U = in.U;
    if (!in.depth)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    const rslf_view_counts& c = r.counts ? *r.counts : kNoCounts;
    const void* outs[6] = {c.seen, c.agree, c.above, c.below, r.fused, r.valid_out};
    bool any = false, aliased = false;
    for (const void* o : outs) {
        any = any || o != nullptr;
        aliased = aliased || (o != nullptr && (o == in.depth || o == in.valid));
    }
    switch (plan::consistency_args(S, V, U, r.tol, r.min_agree, any, aliased)) {
    case plan::kConsistencyOk:
        break;
    case plan::kConsistencyBadShape:
        return fail(RSLF_ERR_INVALID_ARG, "S=%d V=%d U=%d: not a stack of planes", S, V, U);
    case plan::kConsistencyBadTol:
        return fail(RSLF_ERR_INVALID_ARG, "tol=%g: a finite tolerance >= 0", (double)r.tol);
    case plan::kConsistencyBadMinAgree:
        return fail(RSLF_ERR_INVALID_ARG, "min_agree=%d: a count of views >= 0", r.min_agree);
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

// One launch on the context's stream, writing device planes; arguments checked.
int launch_consistency(rslf_ctx* ctx, unsigned grid, const StackIn& in, const Request& r, const rslf_view_counts& c, float* fused,
                       uint8_t* valid_out)
{
    ConsistencyArgs a = {};
    a.depth = in.depth, a.valid = in.valid;
    a.S = in.S, a.V = in.V, a.U = in.U, a.nseg = plan::consistency_segments(in.U);
    a.slope = in.slope, a.tol = r.tol, a.radius = r.radius, a.min_agree = r.min_agree;
    a.order = ctx->consistency_order;
    a.seen = c.seen, a.agree = c.agree, a.above = c.above, a.below = c.below;
    a.fused = fused, a.valid_out = valid_out;
    if (in.valid)
        hipLaunchKernelGGL(k12_view_consistency<true>, dim3(grid), dim3(plan::kConsistencyBlock), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(k12_view_consistency<false>, dim3(grid), dim3(plan::kConsistencyBlock), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

// The checks, then the launch.  host_in: the input planes are host memory; host: the result planes are -- in the output stage
// the 4-byte planes one after the other, the byte plane last, packed.
int consistency(rslf_ctx* ctx, StackIn in, const Request& r, bool host_in, bool host)
{
    unsigned grid = 0;
    int rc = check_consistency_args(in, r, &grid);
    if (!rc)
        rc = begin_stack(ctx, host);
    if (!rc && host_in)
        rc = stage_stack_in(ctx, in.depth, in.valid, in.S, in.V, in.U, &in);
    if (rc)
        return rc;
    const rslf_view_counts& c = r.counts ? *r.counts : kNoCounts;
    if (!host)
        return launch_consistency(ctx, grid, in, r, c, r.fused, r.valid_out);
    const size_t n = (size_t)in.S * in.V * in.U;
    const HostPlane planes[6] = {{c.seen, n * 4}, {c.agree, n * 4}, {c.above, n * 4}, {c.below, n * 4}, {r.fused, n * 4}, {r.valid_out, n}};
    void* dev[6];
    rc = stage_out(ctx, planes, 6, 1, dev);
    if (rc)
        return rc;
    const rslf_view_counts dc = {static_cast<int32_t*>(dev[0]), static_cast<int32_t*>(dev[1]), static_cast<int32_t*>(dev[2]),
                                 static_cast<int32_t*>(dev[3])};
    rc = launch_consistency(ctx, grid, in, r, dc, static_cast<float*>(dev[4]), static_cast<uint8_t*>(dev[5]));
    return deliver_out(ctx, rc, planes, 6, dev);
}

}  // namespace

extern "C" int rslf_view_consistency(rslf_ctx* ctx, const float* d_depth_svu, const uint8_t* d_valid_svu, int S, int V, int U, float slope,
                                     float tol, int radius, int min_agree, const rslf_view_counts* d_out, float* d_fused_svu,
                                     uint8_t* d_valid_out_svu) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    return consistency(ctx, {d_depth_svu, d_valid_svu, S, V, U, slope, nullptr}, {tol, radius, min_agree, d_out, d_fused_svu, d_valid_out_svu},
                       false, false);
}
RSLF_API_CATCH

extern "C" int rslf_view_consistency_host(rslf_ctx* ctx, const float* h_depth_svu, const uint8_t* h_valid_svu, int S, int V, int U,
                                          float slope, float tol, int radius, int min_agree, const rslf_view_counts* h_out,
                                          float* h_fused_svu, uint8_t* h_valid_out_svu) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    return consistency(ctx, {h_depth_svu, h_valid_svu, S, V, U, slope, nullptr}, {tol, radius, min_agree, h_out, h_fused_svu, h_valid_out_svu},
                       true, true);
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
extern "C" int rslf_f2c_run_consistency(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, float tol, int radius,
                                        int min_agree, const rslf_view_counts* d_out, float* d_fused_svu,
                                        uint8_t* d_valid_out_svu) RSLF_API_TRY
{
    StackIn in;
    if (int rc = kept_stack(run, ctx, level, fused_result, &in))
        return rc;
    return consistency(ctx, in, {tol, radius, min_agree, d_out, d_fused_svu, d_valid_out_svu}, false, false);
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_consistency_host(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, float tol, int radius,
                                             int min_agree, const rslf_view_counts* h_out, float* h_fused_svu,
                                             uint8_t* h_valid_out_svu) RSLF_API_TRY
{
    StackIn in;
    if (int rc = kept_stack(run, ctx, level, fused_result, &in))
        return rc;
    return consistency(ctx, in, {tol, radius, min_agree, h_out, h_fused_svu, h_valid_out_svu}, false, true);
}
RSLF_API_CATCH
