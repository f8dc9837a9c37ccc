// The host frame of the operations on a sweep's [S][V][U] disparity planes -- cross-view consistency (rslf_consistency.hip),
// the view warp (rslf_warp.hip), the novel view (rslf_novel.hip) --, each with four C entries: planes on the device, planes on
// the host, a kept fine-to-coarse run read in place, and the kept run with its outputs on the host.  What the four forms of
// every operation share is stated here once: where the inputs come from (StackIn, kept_stack, stage_stack_in), what a form
// does before it queues anything (begin_stack), and how host outputs travel (stage_out, deliver_out).  The device forms
// enqueue on the context's stream and return; the host forms refuse an open sweep (they use the shared stage buffers, which
// the sweep's visits share), stage through kSharedStagePlanes / kSharedStageMask / kSharedStageOut, and wait for the stream,
// after a failed launch too.  Then the pieces the warp and the novel view share.  Host code only, no kernels.
#pragma once

#include "rslf_internal.hpp"
#include "rslf_plan_stage.hpp"
#include "rslf_plan_warp.hpp"

namespace rslf {

// The device-side inputs of a stack operation, wherever they came from (before stage_stack_in: the caller's host planes).
struct StackIn {
    const float* depth;
    const uint8_t* valid;   // nullable: every pixel
    int S, V, U;
    float slope;
    const rslf_volume* vol;   // nullable
};

// A kept run's plane pair -- the fused map and its validity (fused_result, which needs level 0) or a level's depth / valid --,
// the slope factor the level's sweep propagated with (f2c.hpp:139; the fused planes are level 0's size: its factor) and the
// level's kept volume, NULL in a run made without keep_volumes.
inline int kept_stack(const rslf_f2c_run* run, const rslf_ctx* ctx, int level, int fused_result, StackIn* in)
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
    in->depth = fused_result ? run->kept.fused_map.as<const float>() : kl.depth.as<const float>();
    in->valid = fused_result ? run->kept.fused_valid.as<const uint8_t>() : kl.valid.as<const uint8_t>();
    in->S = run->S, in->V = kl.V, in->U = kl.U;
    in->slope = kl.slope;
    in->vol = run->options.keep_volumes ? kl.vol.get() : nullptr;
    return RSLF_OK;
}

// What every form does after the operation's argument checks and before it queues anything.
inline int begin_stack(rslf_ctx* ctx, bool host)
{
    if (host && ctx->sweep.open)
        return fail(RSLF_ERR_INVALID_ARG, "a sweep is open on this context");
    HIP_TRY(hipSetDevice(ctx->device));
    return RSLF_OK;
}

// Host planes into the context's shared stage buffers, queued on its stream: *in reads them there.
inline int stage_stack_in(rslf_ctx* ctx, const float* h_depth, const uint8_t* h_valid, int S, int V, int U, StackIn* in)
{
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)S * V * U;
    void *d_depth = nullptr, *d_valid = nullptr;
    int rc = helper_scratch(ctx, kSharedStagePlanes, n * sizeof(float), &d_depth);
    if (!rc && h_valid)
        rc = helper_scratch(ctx, kSharedStageMask, n, &d_valid);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpyAsync(d_depth, h_depth, n * sizeof(float), hipMemcpyHostToDevice, st));
    if (h_valid)
        HIP_TRY(hipMemcpyAsync(d_valid, h_valid, n, hipMemcpyHostToDevice, st));
    in->depth = static_cast<const float*>(d_depth), in->valid = static_cast<const uint8_t*>(d_valid);
    in->S = S, in->V = V, in->U = U;
    return RSLF_OK;
}

// One output plane of a host form: the caller's pointer (NULL: not asked for) and the plane's size.
struct HostPlane {
    void* host;
    size_t bytes;
};
constexpr int kMaxHostPlanes = 16;

// The planes asked for laid out in the context's shared output buffer (plan::stage_layout): dev[i] is where the launch writes
// plane i, NULL for a plane not asked for.
inline int stage_out(rslf_ctx* ctx, const HostPlane* planes, int n, size_t align, void** dev)
{
    size_t bytes[kMaxHostPlanes], offsets[kMaxHostPlanes];
    bool wanted[kMaxHostPlanes];
    for (int i = 0; i < n; i++)
        bytes[i] = planes[i].bytes, wanted[i] = planes[i].host != nullptr;
    const size_t total = plan::stage_layout(bytes, wanted, n, align, offsets);
    if (total == plan::kStageTooLarge)
        return fail(RSLF_ERR_UNSUPPORTED, "the output planes asked for are larger than the address space");
    void* d_stage = nullptr;
    int rc = helper_scratch(ctx, kSharedStageOut, total, &d_stage);
    for (int i = 0; i < n; i++)
        dev[i] = !rc && wanted[i] ? static_cast<char*>(d_stage) + offsets[i] : nullptr;
    return rc;
}

// ... and after the launches (launch_rc: their status): a failed launch is waited for and its status returned; else the planes
// are copied out and the stream awaited.
inline int deliver_out(rslf_ctx* ctx, int launch_rc, const HostPlane* planes, int n, void* const* dev)
{
    hipStream_t st = ctx->stream;
    if (launch_rc) {
        (void)hipStreamSynchronize(st);
        return launch_rc;
    }
    for (int i = 0; i < n; i++)
        if (planes[i].host && planes[i].bytes)
            HIP_TRY(hipMemcpyAsync(planes[i].host, dev[i], planes[i].bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RSLF_OK;
}

inline int check_volume_device(const rslf_ctx* ctx, const rslf_volume* vol)
{
    if (vol && vol->device != ctx->device)
        return fail(RSLF_ERR_INVALID_ARG, "volume lives on device %d, the context on device %d", vol->device, ctx->device);
    return RSLF_OK;
}

// ---- the warp family: the view warp and the novel view -----------------------------------------------------------------

// The argument checks the two share (plan::warp_args, plan::warp_limits and plan::warp_target_arg name the fault), in the
// order they are made.  outs: the n_outs output planes; needs_volume: colour, err or row_err is among them; needs_views: err
// or row_err is.  count_word, zbuf_owner: the operation's own words.  between (nullable): the operation's own argument check,
// made after the shared arguments and before the limits.
inline int check_warp_family_args(const StackIn& in, const float* targets, int T, int nearer, bool needs_volume, bool needs_views,
                                  const void* const* outs, int n_outs, const char* count_word, const char* zbuf_owner,
                                  const std::function<int()>& between = nullptr)
{
    const int S = in.S, V = in.V, U = in.U;
    const rslf_volume* vol = in.vol;
    if (!in.depth)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument: the depth plane");
    bool any = false, aliased = false;
    for (int i = 0; i < n_outs; i++) {
        const void* p = outs[i];
        any = any || p != nullptr;
        aliased = aliased || (p != nullptr && (p == in.depth || p == in.valid || (vol && p == (const void*)vol->base)));
    }
    switch (plan::warp_args(S, V, U, T, nearer, any, aliased, needs_volume, vol != nullptr, vol ? vol->V : 0, vol ? vol->S : 0, vol ? vol->U : 0)) {
    case plan::kWarpOk:
        break;
    case plan::kWarpBadShape:
        return fail(RSLF_ERR_INVALID_ARG, "S=%d V=%d U=%d: not a stack of planes", S, V, U);
    case plan::kWarpBadTargets:
        return fail(RSLF_ERR_INVALID_ARG, "T=%d: at least one target", T);
    case plan::kWarpBadNearer:
        return fail(RSLF_ERR_INVALID_ARG, "nearer=0: +1 (larger disparities are nearer) or -1");
    case plan::kWarpNoOutput:
        return fail(RSLF_ERR_INVALID_ARG, "all %s output planes are NULL, nothing to compute", count_word);
    case plan::kWarpAlias:
        return fail(RSLF_ERR_INVALID_ARG, "an output plane is an input plane");
    case plan::kWarpNoVolume:
        return fail(RSLF_ERR_INVALID_ARG, "colour, err and row_err read the light field: volume is NULL");
    case plan::kWarpVolumeShape:
        return fail(RSLF_ERR_INVALID_ARG, "volume is V=%d S=%d U=%d, the planes S=%d V=%d U=%d", vol->V, vol->S, vol->U, S, V, U);
    }
    if (between)
        if (int rc = between())
            return rc;
    switch (plan::warp_limits(S, V, U, T)) {
    case plan::kWarpFits:
        break;
    case plan::kWarpTooWide:
        return fail(RSLF_ERR_UNSUPPORTED, "rows of U=%d columns: %s z-buffer holds %d", U, zbuf_owner, plan::kWarpMaxU);
    case plan::kWarpTooManyViews:
        return fail(RSLF_ERR_UNSUPPORTED, "S=%d views: the warp's keys count %d", S, kWarpMaxViews);
    case plan::kWarpGridLimit:
        return fail(RSLF_ERR_UNSUPPORTED, "T=%d V=%d exceed the grid limit of one launch", T, V);
    }
    if (!targets)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument: targets");
    if (needs_volume && !vol->filled)
        return fail(RSLF_ERR_INVALID_ARG, "volume has not been filled");
    for (int k = 0; k < T; k++)
        switch (plan::warp_target_arg(targets[k], S, needs_views)) {
        case plan::kWarpTargetOk:
            break;
        case plan::kWarpTargetRange:
            return fail(RSLF_ERR_INVALID_ARG, "targets[%d]=%g: a finite position within +-65536", k, (double)targets[k]);
        case plan::kWarpTargetNotAView:
            return fail(RSLF_ERR_INVALID_ARG, "targets[%d]=%g: err compares with the view that was taken, a view index in [0, %d)", k,
                        (double)targets[k], S);
        }
    return RSLF_OK;
}

// The refusal of the kept-run forms of both: a plane that reads the level's volume, asked of a run that kept none.
inline int check_kept_volume(const StackIn& in, bool needs_volume)
{
    if (!in.vol && needs_volume)
        return fail(RSLF_ERR_INVALID_ARG, "colour, err and row_err read the level's volume: the run was made without keep_volumes");
    return RSLF_OK;
}

// The launches of a call, plan::kWarpLaunchTargets targets each: `a` (WarpArgs / NovelArgs, the operation's own fields and
// output planes set) gets the inputs, the volume when a plane reads it, `vec` -- rows of whole float4s and every one of the
// first n_vec planes of outs on a 16-byte boundary (the planes after them are written one value at a time) -- and per launch
// its targets; launch(grid, a) queues one.  targets / exclude are read before the return.
template <typename Args, typename Launch>
int launch_warp_family(Args& a, const StackIn& in, bool needs_volume, const float* targets, const int* exclude, int T, const void* const* outs,
                       int n_vec, Launch launch)
{
    a.depth = in.depth, a.valid = in.valid;
    a.S = in.S, a.V = in.V, a.U = in.U;
    a.slope = in.slope;
    if (in.vol && needs_volume)
        a.vol = view_of(in.vol);
    bool aligned = in.U % 4 == 0;
    for (int i = 0; i < n_vec; i++)
        aligned = aligned && (reinterpret_cast<uintptr_t>(outs[i]) & 15u) == 0;
    a.vec = aligned ? 1 : 0;
    for (int l = 0; l < plan::warp_launches(T); l++) {
        a.k_first = l * plan::kWarpLaunchTargets;
        a.T = plan::warp_launch_targets(T, l);
        for (int k = 0; k < a.T; k++) {
            a.target[k] = targets[a.k_first + k];
            a.exclude[k] = exclude ? exclude[a.k_first + k] : -1;
        }
        if (int rc = launch(plan::warp_grid(in.V, a.T), a))
            return rc;
    }
    return RSLF_OK;
}

}  // namespace rslf
