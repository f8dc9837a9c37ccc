// librslf_hip.so: the novel view (K15, k15_novel_view.hpp) -- rslf_novel_view on planes the caller holds on the device,
// rslf_novel_view_host, which stages host planes through the context's shared buffers, and rslf_f2c_run_novel_view (with its
// host-output form), which reads a kept fine-to-coarse run's planes and kept volume in place.  The four forms' frame and what
// the novel view shares with the warp: rslf_stack_op.hpp.  C-ABI: include/rslf_hip.h.  One device.
#include "rslf_internal.hpp"
#include "rslf_plan_novel.hpp"
#include "rslf_stack_op.hpp"

#include "k15_novel_view.hpp"

using namespace rslf;

namespace {

const rslf_novel_view_out kNoPlanes = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
constexpr int kPlanes = 7;

// What a call asks for besides its inputs.
struct Request {
    const float* targets;
    const int* exclude;
    int T;
    const rslf_novel_view_params* p;
    const rslf_novel_view_out* out;   // nullable: none of the seven
};

// The warp family's checks with the novel view's own (plan::novel_args names the fault) among them.
int check_novel_args(const StackIn& in, const Request& r)
{
    const rslf_novel_view_params* p = r.p;
    if (!p)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument: params");
    const rslf_novel_view_out& o = r.out ? *r.out : kNoPlanes;
    const void* outs[kPlanes] = {o.colour, o.depth, o.fill, o.n_src, o.err, o.row_err, o.row_cov};
    const auto own_args = [p]() -> int {
        switch (plan::novel_args(true, p->sources, p->tol)) {
        case plan::kNovelOk:
        case plan::kNovelNoParams:
            break;
        case plan::kNovelBadSources:
            return fail(RSLF_ERR_INVALID_ARG, "sources=%d: at least one view to blend", p->sources);
        case plan::kNovelBadTol:
            return fail(RSLF_ERR_INVALID_ARG, "tol=%g: a tolerance is not negative and not a NaN", (double)p->tol);
        }
        return RSLF_OK;
    };
    return check_warp_family_args(in, r.targets, r.T, p->nearer, o.colour || o.err || o.row_err, o.err || o.row_err, outs, kPlanes, "seven",
                                  "the novel view's", own_args);
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

// The launches of a call on the context's stream, writing the device planes o; arguments checked.
int launch_novel(rslf_ctx* ctx, const StackIn& in, const Request& r, const rslf_novel_view_out& o)
{
    const rslf_novel_view_params& p = *r.p;
    NovelArgs a = {};
    a.radius = p.radius, a.nearer = p.nearer, a.max_gap = p.max_gap, a.sources = p.sources, a.tol = p.tol;
    a.colour = o.colour, a.out_depth = o.depth, a.fill = o.fill, a.n_src = o.n_src, a.err = o.err, a.row_err = o.row_err, a.row_cov = o.row_cov;
    const void* outs[kPlanes] = {o.colour, o.depth, o.fill, o.n_src, o.err, o.row_err, o.row_cov};
    const size_t lds = plan::novel_lds_bytes(in.U);
    const bool valid = in.valid != nullptr;
    return launch_warp_family(a, in, o.colour || o.err || o.row_err, r.targets, r.exclude, r.T, outs, 5, [&](unsigned grid, const NovelArgs& w) {
        return valid ? launch_channels<true>(ctx->stream, grid, lds, w) : launch_channels<false>(ctx->stream, grid, lds, w);
    });
}

// The checks, then the launches.  host_in: the input planes are host memory; host: the result planes are -- each at a 16-byte
// boundary of the output stage.
int novel_view(rslf_ctx* ctx, StackIn in, const Request& r, bool host_in, bool host)
{
    int rc = check_novel_args(in, r);
    if (!rc)
        rc = check_volume_device(ctx, in.vol);   // (the caller's; a kept run's is on the run's device, which kept_stack checked)
    if (!rc)
        rc = begin_stack(ctx, host);
    if (!rc && host_in)
        rc = stage_stack_in(ctx, in.depth, in.valid, in.S, in.V, in.U, &in);
    if (rc)
        return rc;
    const rslf_novel_view_out& h = r.out ? *r.out : kNoPlanes;
    if (!host)
        return launch_novel(ctx, in, r, h);
    const size_t n = (size_t)r.T * in.V * in.U, rows = (size_t)r.T * in.V, C = in.vol ? (size_t)in.vol->C : 0;
    const HostPlane planes[kPlanes] = {{h.colour, n * 4 * C}, {h.depth, n * 4},      {h.fill, n},          {h.n_src, n * 4},
                                       {h.err, n * 4},        {h.row_err, rows * 8}, {h.row_cov, rows * 4}};
    void* dev[kPlanes];
    rc = stage_out(ctx, planes, kPlanes, 16, dev);
    if (rc)
        return rc;
    const rslf_novel_view_out d = {static_cast<float*>(dev[0]),   static_cast<float*>(dev[1]), static_cast<uint8_t*>(dev[2]),
                                   static_cast<int32_t*>(dev[3]), static_cast<float*>(dev[4]), static_cast<double*>(dev[5]),
                                   static_cast<int32_t*>(dev[6])};
    return deliver_out(ctx, launch_novel(ctx, in, r, d), planes, kPlanes, dev);
}

// rslf_f2c_run_novel_view and its host form: the kept planes and the level's kept volume are read in place
int run_novel_view(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, const Request& r, bool host)
{
    StackIn in;
    int rc = kept_stack(run, ctx, level, fused_result, &in);
    if (!rc)
        rc = check_kept_volume(in, r.out && (r.out->colour || r.out->err || r.out->row_err));
    return rc ? rc : novel_view(ctx, in, r, false, host);
}

}  // namespace

extern "C" int rslf_novel_view(rslf_ctx* ctx, const float* d_depth_svu, const uint8_t* d_valid_svu, int S, int V, int U, float slope,
                               const rslf_volume* volume, const float* targets, const int* exclude, int T,
                               const rslf_novel_view_params* params, const rslf_novel_view_out* d_out) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    return novel_view(ctx, {d_depth_svu, d_valid_svu, S, V, U, slope, volume}, {targets, exclude, T, params, d_out}, false, false);
}
RSLF_API_CATCH

extern "C" int rslf_novel_view_host(rslf_ctx* ctx, const float* h_depth_svu, const uint8_t* h_valid_svu, int S, int V, int U, float slope,
                                    const rslf_volume* volume, const float* targets, const int* exclude, int T,
                                    const rslf_novel_view_params* params, const rslf_novel_view_out* h_out) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    return novel_view(ctx, {h_depth_svu, h_valid_svu, S, V, U, slope, volume}, {targets, exclude, T, params, h_out}, true, true);
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_novel_view(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, const float* targets,
                                       const int* exclude, int T, const rslf_novel_view_params* params,
                                       const rslf_novel_view_out* d_out) RSLF_API_TRY
{
    return run_novel_view(run, ctx, level, fused_result, {targets, exclude, T, params, d_out}, false);
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_novel_view_host(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, const float* targets,
                                            const int* exclude, int T, const rslf_novel_view_params* params,
                                            const rslf_novel_view_out* h_out) RSLF_API_TRY
{
    return run_novel_view(run, ctx, level, fused_result, {targets, exclude, T, params, h_out}, true);
}
RSLF_API_CATCH
