// librslf_hip.so: the view warp (K14, k14_view_warp.hpp) -- rslf_view_warp on planes the caller holds on the device,
// rslf_view_warp_host, which stages host planes through the context's shared buffers, and rslf_f2c_run_view_warp (with its
// host-output form), which reads a kept fine-to-coarse run's planes and kept volume in place.  The four forms' frame and what
// the warp shares with the novel view: rslf_stack_op.hpp.  C-ABI: include/rslf_hip.h.  One device.
#include "rslf_internal.hpp"
#include "rslf_stack_op.hpp"

#include "k14_view_warp.hpp"

using namespace rslf;

namespace {

const rslf_view_warp_out kNoPlanes = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
constexpr int kPlanes = 9;

// What a call asks for besides its inputs.
struct Request {
    const float* targets;
    const int* exclude;
    int T, radius, nearer;
    const rslf_view_warp_out* out;   // nullable: none of the nine
};

int check_warp_args(const StackIn& in, const Request& r)
{
    const rslf_view_warp_out& o = r.out ? *r.out : kNoPlanes;
    const void* outs[kPlanes] = {o.hit, o.depth, o.src_view, o.src_col, o.count, o.colour, o.err, o.row_err, o.row_hits};
    return check_warp_family_args(in, r.targets, r.T, r.nearer, o.colour || o.err || o.row_err, o.err || o.row_err, outs, kPlanes, "nine",
                                  "the warp's");
}

template <bool HAS_VALID, bool COUNT>
int launch_one(hipStream_t st, unsigned grid, size_t lds, const WarpArgs& a)
{
    // (more than the 64 KiB a kernel gets without asking: set on every launch)
    if (lds > ((size_t)64 << 10))
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k14_view_warp<HAS_VALID, COUNT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
    hipLaunchKernelGGL((k14_view_warp<HAS_VALID, COUNT>), dim3(grid), dim3(plan::kWarpBlock), lds, st, a);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

// The launches of a call on the context's stream, writing the device planes o; arguments checked.
int launch_warp(rslf_ctx* ctx, const StackIn& in, const Request& r, const rslf_view_warp_out& o)
{
    WarpArgs a = {};
    a.radius = r.radius, a.nearer = r.nearer;
    a.hit = o.hit, a.out_depth = o.depth, a.src_view = o.src_view, a.src_col = o.src_col, a.count = o.count;
    a.colour = o.colour, a.err = o.err, a.row_err = o.row_err, a.row_hits = o.row_hits;
    const void* outs[kPlanes] = {o.hit, o.depth, o.src_view, o.src_col, o.count, o.colour, o.err, o.row_err, o.row_hits};
    const size_t lds = plan::warp_lds_bytes(in.U, o.count != nullptr);
    const bool valid = in.valid != nullptr, count = o.count != nullptr;
    return launch_warp_family(a, in, o.colour || o.err || o.row_err, r.targets, r.exclude, r.T, outs, 7, [&](unsigned grid, const WarpArgs& w) {
        if (valid)
            return count ? launch_one<true, true>(ctx->stream, grid, lds, w) : launch_one<true, false>(ctx->stream, grid, lds, w);
        return count ? launch_one<false, true>(ctx->stream, grid, lds, w) : launch_one<false, false>(ctx->stream, grid, lds, w);
    });
}

// The checks, then the launches.  host_in: the input planes are host memory; host: the result planes are -- each at a 16-byte
// boundary of the output stage.
int view_warp(rslf_ctx* ctx, StackIn in, const Request& r, bool host_in, bool host)
{
    int rc = check_warp_args(in, r);
    if (!rc)
        rc = check_volume_device(ctx, in.vol);   // (the caller's; a kept run's is on the run's device, which kept_stack checked)
    if (!rc)
        rc = begin_stack(ctx, host);
    if (!rc && host_in)
        rc = stage_stack_in(ctx, in.depth, in.valid, in.S, in.V, in.U, &in);
    if (rc)
        return rc;
    const rslf_view_warp_out& h = r.out ? *r.out : kNoPlanes;
    if (!host)
        return launch_warp(ctx, in, r, h);
    const size_t n = (size_t)r.T * in.V * in.U, rows = (size_t)r.T * in.V, C = in.vol ? (size_t)in.vol->C : 0;
    const HostPlane planes[kPlanes] = {{h.hit, n},         {h.depth, n * 4}, {h.src_view, n * 4},  {h.src_col, n * 4}, {h.count, n * 4},
                                       {h.colour, n * 4 * C}, {h.err, n * 4},   {h.row_err, rows * 8}, {h.row_hits, rows * 4}};
    void* dev[kPlanes];
    rc = stage_out(ctx, planes, kPlanes, 16, dev);
    if (rc)
        return rc;
    const rslf_view_warp_out d = {static_cast<uint8_t*>(dev[0]), static_cast<float*>(dev[1]),  static_cast<int32_t*>(dev[2]),
                                  static_cast<int32_t*>(dev[3]), static_cast<int32_t*>(dev[4]), static_cast<float*>(dev[5]),
                                  static_cast<float*>(dev[6]),   static_cast<double*>(dev[7]),  static_cast<int32_t*>(dev[8])};
    return deliver_out(ctx, launch_warp(ctx, in, r, d), planes, kPlanes, dev);
}

// rslf_f2c_run_view_warp and its host form: the kept planes and the level's kept volume are read in place
int run_view_warp(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, const Request& r, bool host)
{
    StackIn in;
    int rc = kept_stack(run, ctx, level, fused_result, &in);
    if (!rc)
        rc = check_kept_volume(in, r.out && (r.out->colour || r.out->err || r.out->row_err));
    return rc ? rc : view_warp(ctx, in, r, false, host);
}

}  // namespace

extern "C" int rslf_view_warp(rslf_ctx* ctx, const float* d_depth_svu, const uint8_t* d_valid_svu, int S, int V, int U, float slope,
                              const rslf_volume* volume, const float* targets, const int* exclude, int T, int radius, int nearer,
                              const rslf_view_warp_out* d_out) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    return view_warp(ctx, {d_depth_svu, d_valid_svu, S, V, U, slope, volume}, {targets, exclude, T, radius, nearer, d_out}, false, false);
}
RSLF_API_CATCH

extern "C" int rslf_view_warp_host(rslf_ctx* ctx, const float* h_depth_svu, const uint8_t* h_valid_svu, int S, int V, int U, float slope,
                                   const rslf_volume* volume, const float* targets, const int* exclude, int T, int radius, int nearer,
                                   const rslf_view_warp_out* h_out) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    return view_warp(ctx, {h_depth_svu, h_valid_svu, S, V, U, slope, volume}, {targets, exclude, T, radius, nearer, h_out}, true, true);
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_view_warp(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, const float* targets,
                                      const int* exclude, int T, int radius, int nearer, const rslf_view_warp_out* d_out) RSLF_API_TRY
{
    return run_view_warp(run, ctx, level, fused_result, {targets, exclude, T, radius, nearer, d_out}, false);
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_view_warp_host(const rslf_f2c_run* run, rslf_ctx* ctx, int level, int fused_result, const float* targets,
                                           const int* exclude, int T, int radius, int nearer, const rslf_view_warp_out* h_out) RSLF_API_TRY
{
    return run_view_warp(run, ctx, level, fused_result, {targets, exclude, T, radius, nearer, h_out}, true);
}
RSLF_API_CATCH
