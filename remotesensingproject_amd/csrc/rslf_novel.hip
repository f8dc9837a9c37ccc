// librslf_hip.so: the novel view (K15, k15_novel_view.hpp) -- rslf_novel_view on planes the caller holds on the device,
// rslf_novel_view_host, which stages host planes through the context's shared buffers, and rslf_f2c_run_novel_view (with its
// host-output form), which reads a kept fine-to-coarse run's planes and kept volume in place.  C-ABI: include/rslf_hip.h.
// One device.
#include "rslf_internal.hpp"
#include "rslf_plan_novel.hpp"

#include "k15_novel_view.hpp"

using namespace rslf;

namespace {

const rslf_novel_view_out kNoPlanes = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
constexpr int kPlanes = 7;

void plane_list(const rslf_novel_view_out& o, const void* (&p)[kPlanes])
{
    const void* q[kPlanes] = {o.colour, o.depth, o.fill, o.n_src, o.err, o.row_err, o.row_cov};
    for (int i = 0; i < kPlanes; i++)
        p[i] = q[i];
}

// The argument checks every form shares (plan::novel_args, plan::warp_args, plan::warp_target_arg and plan::warp_limits name
// the fault).
int check_novel_args(const void* depth, const void* valid, int S, int V, int U, const rslf_volume* vol, const float* targets, int T,
                     const rslf_novel_view_params* p, const rslf_novel_view_out& o)
{
    if (!p)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument: params");
    if (!depth)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument: the depth plane");
    const void* outs[kPlanes];
    plane_list(o, outs);
    bool any = false, aliased = false;
    for (const void* q : outs) {
        any = any || q != nullptr;
        aliased = aliased || (q != nullptr && (q == depth || q == valid || (vol && q == (const void*)vol->base)));
    }
    const bool needs_volume = o.colour || o.err || o.row_err;
    switch (plan::warp_args(S, V, U, T, p->nearer, any, aliased, needs_volume, vol != nullptr, vol ? vol->V : 0, vol ? vol->S : 0, vol ? vol->U : 0)) {
    case plan::kWarpOk:
        break;
    case plan::kWarpBadShape:
        return fail(RSLF_ERR_INVALID_ARG, "S=%d V=%d U=%d: not a stack of planes", S, V, U);
    case plan::kWarpBadTargets:
        return fail(RSLF_ERR_INVALID_ARG, "T=%d: at least one target", T);
    case plan::kWarpBadNearer:
        return fail(RSLF_ERR_INVALID_ARG, "nearer=0: +1 (larger disparities are nearer) or -1");
    case plan::kWarpNoOutput:
        return fail(RSLF_ERR_INVALID_ARG, "all seven output planes are NULL, nothing to compute");
    case plan::kWarpAlias:
        return fail(RSLF_ERR_INVALID_ARG, "an output plane is an input plane");
    case plan::kWarpNoVolume:
        return fail(RSLF_ERR_INVALID_ARG, "colour, err and row_err read the light field: volume is NULL");
    case plan::kWarpVolumeShape:
        return fail(RSLF_ERR_INVALID_ARG, "volume is V=%d S=%d U=%d, the planes S=%d V=%d U=%d", vol->V, vol->S, vol->U, S, V, U);
    }
    switch (plan::novel_args(true, p->sources, p->tol)) {
    case plan::kNovelOk:
    case plan::kNovelNoParams:
        break;
    case plan::kNovelBadSources:
        return fail(RSLF_ERR_INVALID_ARG, "sources=%d: at least one view to blend", p->sources);
    case plan::kNovelBadTol:
        return fail(RSLF_ERR_INVALID_ARG, "tol=%g: a tolerance is not negative and not a NaN", (double)p->tol);
    }
    switch (plan::warp_limits(S, V, U, T)) {
    case plan::kWarpFits:
        break;
    case plan::kWarpTooWide:
        return fail(RSLF_ERR_UNSUPPORTED, "rows of U=%d columns: the novel view's z-buffer holds %d", U, plan::kWarpMaxU);
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
        switch (plan::warp_target_arg(targets[k], S, o.err || o.row_err)) {
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

template <bool HAS_VALID, int CT>
int launch_one(hipStream_t st, unsigned grid, size_t lds, const NovelArgs& a)
{
    hipLaunchKernelGGL((k15_novel_view<HAS_VALID, CT>), dim3(grid), dim3(plan::kWarpBlock), lds, st, a);   // lds <= 64 KiB: the cap
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

template <bool HAS_VALID>
int launch_channels(hipStream_t st, unsigned grid, size_t lds, const NovelArgs& a)
{
    if (!a.vol.base)
        return launch_one<HAS_VALID, -1>(st, grid, lds, a);
    switch (a.vol.C) {
    case 1:
        return launch_one<HAS_VALID, 1>(st, grid, lds, a);
    case 3:
        return launch_one<HAS_VALID, 3>(st, grid, lds, a);
    default:
        return fail(RSLF_ERR_INTERNAL, "no novel-view kernel for %d channels", a.vol.C);
    }
}

// The launches of a call on the context's stream; arguments checked.  targets / exclude are read before the return.
int launch_novel(rslf_ctx* ctx, const float* depth, const uint8_t* valid, int S, int V, int U, float slope, const rslf_volume* vol,
                 const float* targets, const int* exclude, int T, const rslf_novel_view_params& p, const rslf_novel_view_out& o)
{
    NovelArgs a = {};
    a.depth = depth, a.valid = valid;
    a.S = S, a.V = V, a.U = U;
    a.slope = slope, a.radius = p.radius, a.nearer = p.nearer, a.max_gap = p.max_gap, a.sources = p.sources, a.tol = p.tol;
    if (vol && (o.colour || o.err || o.row_err))
        a.vol = view_of(vol);
    a.colour = o.colour, a.out_depth = o.depth, a.fill = o.fill, a.n_src = o.n_src, a.err = o.err, a.row_err = o.row_err, a.row_cov = o.row_cov;
    const void* outs[kPlanes];
    plane_list(o, outs);
    bool aligned = U % 4 == 0;
    for (int i = 0; i < 5; i++)   // (the two row planes are written one value at a time)
        aligned = aligned && (reinterpret_cast<uintptr_t>(outs[i]) & 15u) == 0;
    a.vec = aligned ? 1 : 0;
    const size_t lds = plan::novel_lds_bytes(U);
    for (int l = 0; l < plan::warp_launches(T); l++) {
        a.k_first = l * plan::kWarpLaunchTargets;
        a.T = plan::warp_launch_targets(T, l);
        for (int k = 0; k < a.T; k++) {
            a.target[k] = targets[a.k_first + k];
            a.exclude[k] = exclude ? exclude[a.k_first + k] : -1;
        }
        const unsigned grid = plan::warp_grid(V, a.T);
        const int rc = valid ? launch_channels<true>(ctx->stream, grid, lds, a) : launch_channels<false>(ctx->stream, grid, lds, a);
        if (rc)
            return rc;
    }
    return RSLF_OK;
}

size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

// The launches on device inputs with the result planes on the HOST: the planes asked for are staged in the context's shared
// output buffer, each at a 16-byte boundary, copied out, and the stream awaited.
int novel_to_host(rslf_ctx* ctx, const float* d_depth, const uint8_t* d_valid, int S, int V, int U, float slope, const rslf_volume* vol,
                  const float* targets, const int* exclude, int T, const rslf_novel_view_params& p, const rslf_novel_view_out& h)
{
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)T * V * U, rows = (size_t)T * V, C = vol ? (size_t)vol->C : 0;
    void* const host[kPlanes] = {h.colour, h.depth, h.fill, h.n_src, h.err, h.row_err, h.row_cov};
    const size_t bytes[kPlanes] = {n * 4 * C, n * 4, n, n * 4, n * 4, rows * 8, rows * 4};
    size_t total = 0;
    for (int i = 0; i < kPlanes; i++)
        total += host[i] ? up16(bytes[i]) : 0;
    void* d_stage = nullptr;
    int rc = helper_scratch(ctx, kSharedStageOut, total, &d_stage);
    if (rc)
        return rc;
    void* dev[kPlanes] = {};
    char* at = static_cast<char*>(d_stage);
    for (int i = 0; i < kPlanes; i++)
        if (host[i]) {
            dev[i] = at;
            at += up16(bytes[i]);
        }
    const rslf_novel_view_out d = {static_cast<float*>(dev[0]),   static_cast<float*>(dev[1]), static_cast<uint8_t*>(dev[2]),
                                   static_cast<int32_t*>(dev[3]), static_cast<float*>(dev[4]), static_cast<double*>(dev[5]),
                                   static_cast<int32_t*>(dev[6])};
    rc = launch_novel(ctx, d_depth, d_valid, S, V, U, slope, vol, targets, exclude, T, p, d);
    if (rc) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    for (int i = 0; i < kPlanes; i++)
        if (host[i] && bytes[i])
            HIP_TRY(hipMemcpyAsync(host[i], dev[i], bytes[i], hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RSLF_OK;
}

int check_volume_device(const rslf_ctx* ctx, const rslf_volume* vol)
{
    if (vol && vol->device != ctx->device)
        return fail(RSLF_ERR_INVALID_ARG, "volume lives on device %d, the context on device %d", vol->device, ctx->device);
    return RSLF_OK;
}

}  // namespace

extern "C" int rslf_novel_view(rslf_ctx* ctx, const float* d_depth_svu, const uint8_t* d_valid_svu, int S, int V, int U, float slope,
                               const rslf_volume* volume, const float* targets, const int* exclude, int T,
                               const rslf_novel_view_params* params, const rslf_novel_view_out* d_out) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    const rslf_novel_view_out& o = d_out ? *d_out : kNoPlanes;
    int rc = check_novel_args(d_depth_svu, d_valid_svu, S, V, U, volume, targets, T, params, o);
    if (!rc)
        rc = check_volume_device(ctx, volume);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return launch_novel(ctx, d_depth_svu, d_valid_svu, S, V, U, slope, volume, targets, exclude, T, *params, o);   // enqueued, not awaited
}
RSLF_API_CATCH

extern "C" int rslf_novel_view_host(rslf_ctx* ctx, const float* h_depth_svu, const uint8_t* h_valid_svu, int S, int V, int U, float slope,
                                    const rslf_volume* volume, const float* targets, const int* exclude, int T,
                                    const rslf_novel_view_params* params, const rslf_novel_view_out* h_out) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    const rslf_novel_view_out& o = h_out ? *h_out : kNoPlanes;
    int rc = check_novel_args(h_depth_svu, h_valid_svu, S, V, U, volume, targets, T, params, o);
    if (!rc)
        rc = check_volume_device(ctx, volume);
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
    return novel_to_host(ctx, static_cast<const float*>(d_depth), static_cast<const uint8_t*>(d_valid), S, V, U, slope, volume, targets, exclude,
                         T, *params, o);
}
RSLF_API_CATCH

// rslf_f2c_run_novel_view and its host form: the kept planes and the level's kept volume are read in place
static int f2c_run_novel_view(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, const float* targets, const int* exclude,
                              int T, const rslf_novel_view_params* params, const rslf_novel_view_out* out, bool host)
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
    const rslf_novel_view_out& o = out ? *out : kNoPlanes;
    const rslf_volume* vol = run->options.keep_volumes ? kl.vol.get() : nullptr;
    if (!vol && (o.colour || o.err || o.row_err))
        return fail(RSLF_ERR_INVALID_ARG, "colour, err and row_err read the level's volume: the run was made without keep_volumes");
    int rc = check_novel_args(depth, valid, run->S, kl.V, kl.U, vol, targets, T, params, o);
    if (rc)
        return rc;
    if (host && ctx->sweep.open)
        return fail(RSLF_ERR_INVALID_ARG, "a sweep is open on this context");
    HIP_TRY(hipSetDevice(ctx->device));
    // the slope factor the level's sweep propagated with; the fused planes are level 0's size: its factor
    if (host)
        return novel_to_host(ctx, depth, valid, run->S, kl.V, kl.U, kl.slope, vol, targets, exclude, T, *params, o);
    return launch_novel(ctx, depth, valid, run->S, kl.V, kl.U, kl.slope, vol, targets, exclude, T, *params, o);
}

extern "C" int rslf_f2c_run_novel_view(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, const float* targets,
                                       const int* exclude, int T, const rslf_novel_view_params* params,
                                       const rslf_novel_view_out* d_out) RSLF_API_TRY
{
    return f2c_run_novel_view(run, ctx, level, fused_result, targets, exclude, T, params, d_out, false);
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_novel_view_host(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, const float* targets,
                                            const int* exclude, int T, const rslf_novel_view_params* params,
                                            const rslf_novel_view_out* h_out) RSLF_API_TRY
{
    return f2c_run_novel_view(run, ctx, level, fused_result, targets, exclude, T, params, h_out, true);
}
RSLF_API_CATCH
