// librslf_hip.so: the per-view equalisation (K19, k19_equalize.hpp) -- rslf_volume_view_stats and rslf_view_stats_dense count
// a view's quantised samples, rslf_equalize_coefficients turns the counts into one (a, b) per view and channel on the host,
// rslf_volume_equalize_views and rslf_volume_apply_view_gains make a new volume y = a x + b, rslf_equalize_views_dense does
// the same in place to a dense raw level of the pyramid on device pointers (equalize_views_raw: the level loop's own call).
// C-ABI: include/rslf_hip.h.  One device.
#include "rslf_internal.hpp"
#include "rslf_plan_equalize.hpp"

#include "k19_equalize.hpp"

using namespace rslf;

namespace {

int shape_fault(plan::EqualizeArg f, int V, int S, int U, int C)
{
    switch (f) {
    case plan::kEqOk:
        return RSLF_OK;
    case plan::kEqBadShape:
        return fail(RSLF_ERR_INVALID_ARG, "bad dimensions V=%d S=%d U=%d C=%d", V, S, U, C);
    case plan::kEqTooLarge:
        return fail(RSLF_ERR_UNSUPPORTED, "V=%d S=%d U=%d: a view's V * U samples are counted exactly up to 2^31 - 1, and a row of "
                    "3 * U floats and the V * S rows are indexed by int", V, S, U);
    }
    return fail(RSLF_ERR_INTERNAL, "unknown equalize fault");
}

// The options of the coefficients, as every entry that takes them checks them.
int options_fault(int S, int C, int mode, int ref_view, int joint, float max_gain)
{
    if (!eq_mode_ok(mode))
        return fail(RSLF_ERR_INVALID_ARG, "equalize mode %d: RSLF_EQUALIZE_GAIN or RSLF_EQUALIZE_AFFINE", mode);
    if (ref_view < -1 || ref_view >= S)
        return fail(RSLF_ERR_INVALID_ARG, "ref_view=%d: -1 (the mean of the views) or a view in [0, %d)", ref_view, S);
    if (!eq_max_gain_ok(max_gain))
        return fail(RSLF_ERR_INVALID_ARG, "max_gain=%g: a finite gain >= 1", (double)max_gain);
    if (joint && C != 3)
        return fail(RSLF_ERR_INVALID_ARG, "joint=%d with C=%d: the joint statistic is the three channels'", joint, C);
    return RSLF_OK;
}

// The joint statistic's own cap on a view's samples (plan::equalize_joint_fits).
int joint_fault(int V, int U, int joint)
{
    if (joint && !plan::equalize_joint_fits(V, U))
        return fail(RSLF_ERR_UNSUPPORTED, "joint with V=%d U=%d: the three channels' sums are added exactly up to %lld samples of a view",
                    V, U, (long long)kEqMaxSamplesJoint);
    return RSLF_OK;
}

// What the volume entries refuse of a source, in the header's order.
int source_fault(const rslf_ctx* ctx, const rslf_volume* src)
{
    if (!src->filled)
        return fail(RSLF_ERR_INVALID_ARG, "the source volume has not been filled");
    if (src->device != ctx->device)
        return fail(RSLF_ERR_INVALID_ARG, "volume lives on device %d, the context on device %d", src->device, ctx->device);
    if (!(src->min_value >= 0.0f) || !eq_hi_ok(src->max_value))
        return fail(RSLF_ERR_UNSUPPORTED, "a volume of range [%g, %g]: the equalisation is built for a non-negative field with a "
                    "finite maximum > 0", (double)src->min_value, (double)src->max_value);
    return shape_fault(plan::equalize_shape(src->V, src->S, src->U, src->C), src->V, src->S, src->U, src->C);
}

// Zeroes d_stats [S][C][3] and enqueues the statistics kernel.  pitch > 0: the volume form.
int launch_stats(hipStream_t st, const float* d_in, int V, int S, int U, int C, int pitch, float hi, unsigned long long* d_stats)
{
    HIP_TRY(hipMemsetAsync(d_stats, 0, (size_t)S * C * kEqStats * sizeof(unsigned long long), st));
    EqualizeStatsArgs a = {};
    a.src = d_in, a.stats = d_stats;
    a.V = V, a.S = S, a.U = U;
    a.row_px = pitch ? pitch : U, a.pitch = pitch;
    a.base_aligned = (pitch || (uintptr_t)d_in % 16 == 0) ? 1 : 0;
    a.tiles_per_row = plan::equalize_tiles_per_row(U);   // (the volume form's pad holds no sample: no tile for it)
    const plan::EqualizeStatsGrid g = plan::equalize_stats_grid(V, S, a.tiles_per_row);
    a.per_view = g.per_view, a.groups = g.groups;
    a.hi = hi, a.k = eq_quant_scale(hi);
    const unsigned grid = plan::equalize_stats_blocks(g);
    if (C == 1)
        hipLaunchKernelGGL((k19_view_stats<1>), dim3(grid), dim3(plan::kEqBlock), 0, st, a);
    else
        hipLaunchKernelGGL((k19_view_stats<3>), dim3(grid), dim3(plan::kEqBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

int launch_apply(hipStream_t st, int C, bool integer, const EqualizeApplyArgs& a)
{
    const unsigned grid = plan::equalize_apply_grid(a.tiles);
    if (C == 1 && integer)
        hipLaunchKernelGGL((k19_equalize_apply<1, true>), dim3(grid), dim3(plan::kEqBlock), 0, st, a);
    else if (C == 1)
        hipLaunchKernelGGL((k19_equalize_apply<1, false>), dim3(grid), dim3(plan::kEqBlock), 0, st, a);
    else if (integer)
        hipLaunchKernelGGL((k19_equalize_apply<3, true>), dim3(grid), dim3(plan::kEqBlock), 0, st, a);
    else
        hipLaunchKernelGGL((k19_equalize_apply<3, false>), dim3(grid), dim3(plan::kEqBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

// The context's statistics buffer, S * C * 3 integers.
int stats_buffer(rslf_ctx* ctx, int S, int C, unsigned long long** out)
{
    HIP_TRY(hip_err(ctx->scratch.eq_stats.reserve((size_t)S * C * kEqStats * sizeof(unsigned long long))));
    *out = ctx->scratch.eq_stats.as<unsigned long long>();
    return RSLF_OK;
}

// The coefficients on the device: copied from the context's own host copy of them, which outlives the copy.
int upload_table(rslf_ctx* ctx, const float* h_a_b, int S, int C, const float** out)
{
    const size_t n = (size_t)S * C * 2;
    HIP_TRY(hip_err(ctx->scratch.eq_table.reserve(n * sizeof(float))));
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // (an earlier copy out of eq_table_host has ended)
    ctx->eq_table_host.assign(h_a_b, h_a_b + n);
    HIP_TRY(hipMemcpyAsync(ctx->scratch.eq_table.get(), ctx->eq_table_host.data(), n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    *out = ctx->scratch.eq_table.as<const float>();
    return RSLF_OK;
}

// Every pair finite?  (the caller's own coefficients, rslf_volume_apply_view_gains)
bool table_finite(const float* h_a_b, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!(h_a_b[i] - h_a_b[i] == 0.0f))
            return false;
    return true;
}

// Statistics of a filled volume into h_stats, awaited.
int volume_stats(rslf_ctx* ctx, const rslf_volume* vol, uint64_t* h_stats)
{
    unsigned long long* d_stats = nullptr;
    if (int rc = stats_buffer(ctx, vol->S, vol->C, &d_stats))
        return rc;
    if (int rc = launch_stats(ctx->stream, vol->base, vol->V, vol->S, vol->U, vol->C, vol->pitch, vol->max_value, d_stats))
        return rc;
    HIP_TRY(hipMemcpyAsync(h_stats, d_stats, (size_t)vol->S * vol->C * kEqStats * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RSLF_OK;
}

// A new volume y = a x + b of a checked source; the coefficients are the caller's h_a_b [S][C][2].
int volume_apply(rslf_ctx* ctx, const rslf_volume* src, const float* h_a_b, rslf_volume** out)
{
    rslf_volume* vol = nullptr;
    int rc = rslf_volume_create(ctx, src->V, src->S, src->U, src->C, &vol);
    if (rc)
        return rc;
    VolumePtr owner(vol);   // freed on every failure below
    EqualizeApplyArgs a = {};
    a.src = src->base, a.dst = vol->base;
    rc = upload_table(ctx, h_a_b, src->S, src->C, &a.a_b);
    if (rc)
        return rc;
    a.tiles_per_row = plan::equalize_tiles_per_row(src->pitch);
    a.tiles = (long long)src->V * src->S * a.tiles_per_row;
    const unsigned grid = plan::equalize_apply_grid(a.tiles);
    rc = range_partials(ctx, grid, &a.partial);
    if (rc)
        return rc;
    a.S = src->S, a.U = src->U;
    a.row_px = src->pitch, a.pitch = src->pitch, a.base_aligned = 1;   // (vol->pitch is the same: the pitch is a function of U)
    a.hi = src->max_value;
    rc = launch_apply(ctx->stream, src->C, false, a);
    if (rc)
        return rc;
    // the new slab's own range, as an upload of it would find it; the two floats are waited for, as the uploads wait for theirs
    rc = volume_range_from_partials(vol, (int)grid);
    if (rc)
        return rc;
    *out = owner.release();
    return RSLF_OK;
}

// The apply pass on a dense level, enqueued: d_out may be d_in.  hi is the element type's own by now.
int apply_dense(rslf_ctx* ctx, const float* d_in, float* d_out, Elem e, int V, int S, int U, int C, float hi, const float* h_a_b)
{
    EqualizeApplyArgs a = {};
    a.src = d_in, a.dst = d_out, a.partial = nullptr;
    if (int rc = upload_table(ctx, h_a_b, S, C, &a.a_b))
        return rc;
    a.tiles_per_row = plan::equalize_tiles_per_row(U);
    a.tiles = (long long)V * S * a.tiles_per_row;
    a.S = S, a.U = U;
    a.row_px = U, a.pitch = 0;
    a.base_aligned = ((uintptr_t)d_in % 16 == 0 && (uintptr_t)d_out % 16 == 0) ? 1 : 0;
    a.hi = hi;
    return launch_apply(ctx->stream, C, e != Elem::F32, a);
}

}  // namespace

// The dense form in place, awaited: statistics, the wait for S * C * 3 integers, coefficients on the host, apply.
// hi: the cap of float elements; an integer type's own otherwise.  h_a_b [S][C][2], nullable.
int rslf::equalize_views_raw(rslf_ctx* ctx, float* d_inout, Elem e, int V, int S, int U, int C, float hi, int mode, int ref_view, int joint,
                             float max_gain, float* h_a_b)
{
    if (e != Elem::F32)
        hi = eq_hi_int((int)elem_bytes(e));
    unsigned long long* d_stats = nullptr;
    if (int rc = stats_buffer(ctx, S, C, &d_stats))
        return rc;
    if (int rc = launch_stats(ctx->stream, d_inout, V, S, U, C, 0, hi, d_stats))
        return rc;
    std::vector<uint64_t> stats((size_t)S * C * kEqStats);
    HIP_TRY(hipMemcpyAsync(stats.data(), d_stats, stats.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<float> a_b((size_t)S * C * 2);
    eq_coefficients(stats.data(), S, C, hi, mode, ref_view, joint, max_gain, a_b.data());
    if (int rc = apply_dense(ctx, d_inout, d_inout, e, V, S, U, C, hi, a_b.data()))
        return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (h_a_b)
        memcpy(h_a_b, a_b.data(), a_b.size() * sizeof(float));
    return RSLF_OK;
}

int rslf::check_equalize(const F2cOptions& o, int V, int S, int U, int C)
{
    if (o.equalize_mode == 0)
        return RSLF_OK;
    if (int rc = options_fault(S, C, o.equalize_mode, o.equalize_ref_view, o.equalize_joint, o.equalize_max_gain))
        return rc;
    if (int rc = shape_fault(plan::equalize_shape(V, S, U, C), V, S, U, C))
        return rc;
    return joint_fault(V, U, o.equalize_joint);
}

extern "C" int rslf_equalize_coefficients(const uint64_t* h_stats, int S, int C, float hi, int mode, int ref_view, int joint, float max_gain,
                                          float* h_a_b) RSLF_API_TRY
{
    if (!h_stats || !h_a_b)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (S < 1 || (C != 1 && C != 3))
        return fail(RSLF_ERR_INVALID_ARG, "bad dimensions S=%d C=%d", S, C);
    if (!eq_hi_ok(hi))
        return fail(RSLF_ERR_INVALID_ARG, "hi=%g: the cap is finite and > 0", (double)hi);
    if (int rc = options_fault(S, C, mode, ref_view, joint, max_gain))
        return rc;
    eq_coefficients(h_stats, S, C, hi, mode, ref_view, joint, max_gain, h_a_b);
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_volume_view_stats(rslf_ctx* ctx, const rslf_volume* vol, uint64_t* h_stats, float* hi_used) RSLF_API_TRY
{
    if (!ctx || !vol || !h_stats)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (int rc = source_fault(ctx, vol))
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = volume_stats(ctx, vol, h_stats))
        return rc;
    if (hi_used)
        *hi_used = vol->max_value;
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_view_stats_dense(rslf_ctx* ctx, const float* d_in_vsuc, int elem, int V, int S, int U, int C, float hi,
                                     uint64_t* d_stats) RSLF_API_TRY
{
    if (!ctx || !d_in_vsuc || !d_stats)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    Elem e;
    if (int rc = elem_of(elem, &e))
        return rc;
    if (e == Elem::F32 && !eq_hi_ok(hi))
        return fail(RSLF_ERR_INVALID_ARG, "hi=%g: the cap of float elements is finite and > 0", (double)hi);
    if ((uintptr_t)d_stats % 8 != 0)
        return fail(RSLF_ERR_INVALID_ARG, "d_stats is not 8-byte aligned");
    if (int rc = shape_fault(plan::equalize_shape(V, S, U, C), V, S, U, C))
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (e != Elem::F32)
        hi = eq_hi_int((int)elem_bytes(e));
    return launch_stats(ctx->stream, d_in_vsuc, V, S, U, C, 0, hi, reinterpret_cast<unsigned long long*>(d_stats));   // enqueued, not awaited
}
RSLF_API_CATCH

extern "C" int rslf_volume_equalize_views(rslf_ctx* ctx, const rslf_volume* src, int mode, int ref_view, int joint, float max_gain,
                                          rslf_volume** out, float* h_a_b) RSLF_API_TRY
{
    if (!out)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument: out");
    if (src && *out == src)   // (the caller's one handle of the source: left as it is)
        return fail(RSLF_ERR_INVALID_ARG, "out holds the source volume: the call would overwrite its handle");
    *out = nullptr;
    if (!ctx || !src)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (int rc = options_fault(src->S, src->C, mode, ref_view, joint, max_gain))
        return rc;
    if (int rc = source_fault(ctx, src))
        return rc;
    if (int rc = joint_fault(src->V, src->U, joint))
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<uint64_t> stats((size_t)src->S * src->C * kEqStats);
    if (int rc = volume_stats(ctx, src, stats.data()))
        return rc;
    std::vector<float> a_b((size_t)src->S * src->C * 2);
    eq_coefficients(stats.data(), src->S, src->C, src->max_value, mode, ref_view, joint, max_gain, a_b.data());
    if (int rc = volume_apply(ctx, src, a_b.data(), out))
        return rc;
    if (h_a_b)
        memcpy(h_a_b, a_b.data(), a_b.size() * sizeof(float));
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_volume_apply_view_gains(rslf_ctx* ctx, const rslf_volume* src, const float* h_a_b, rslf_volume** out) RSLF_API_TRY
{
    if (!out)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument: out");
    if (src && *out == src)
        return fail(RSLF_ERR_INVALID_ARG, "out holds the source volume: the call would overwrite its handle");
    *out = nullptr;
    if (!ctx || !src || !h_a_b)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (int rc = source_fault(ctx, src))
        return rc;
    if (!table_finite(h_a_b, (size_t)src->S * src->C * 2))
        return fail(RSLF_ERR_INVALID_ARG, "h_a_b holds a coefficient that is not finite");
    HIP_TRY(hipSetDevice(ctx->device));
    return volume_apply(ctx, src, h_a_b, out);
}
RSLF_API_CATCH

extern "C" int rslf_equalize_views_dense(rslf_ctx* ctx, float* d_inout_vsuc, int elem, int V, int S, int U, int C, float hi, int mode,
                                         int ref_view, int joint, float max_gain, float* h_a_b) RSLF_API_TRY
{
    if (!ctx || !d_inout_vsuc)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    Elem e;
    if (int rc = elem_of(elem, &e))
        return rc;
    if (e == Elem::F32 && !eq_hi_ok(hi))
        return fail(RSLF_ERR_INVALID_ARG, "hi=%g: the cap of float elements is finite and > 0", (double)hi);
    if (int rc = shape_fault(plan::equalize_shape(V, S, U, C), V, S, U, C))
        return rc;
    if (int rc = options_fault(S, C, mode, ref_view, joint, max_gain))
        return rc;
    if (int rc = joint_fault(V, U, joint))
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return equalize_views_raw(ctx, d_inout_vsuc, e, V, S, U, C, hi, mode, ref_view, joint, max_gain, h_a_b);
}
RSLF_API_CATCH

extern "C" int rslf_apply_view_gains_dense(rslf_ctx* ctx, const float* d_in_vsuc, int elem, int V, int S, int U, int C, float hi,
                                           const float* h_a_b, float* d_out_vsuc) RSLF_API_TRY
{
    if (!ctx || !d_in_vsuc || !h_a_b || !d_out_vsuc)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    Elem e;
    if (int rc = elem_of(elem, &e))
        return rc;
    if (e == Elem::F32 && !eq_hi_ok(hi))
        return fail(RSLF_ERR_INVALID_ARG, "hi=%g: the cap of float elements is finite and > 0", (double)hi);
    if (int rc = shape_fault(plan::equalize_shape(V, S, U, C), V, S, U, C))
        return rc;
    if (!table_finite(h_a_b, (size_t)S * C * 2))
        return fail(RSLF_ERR_INVALID_ARG, "h_a_b holds a coefficient that is not finite");
    HIP_TRY(hipSetDevice(ctx->device));
    if (e != Elem::F32)
        hi = eq_hi_int((int)elem_bytes(e));
    return apply_dense(ctx, d_in_vsuc, d_out_vsuc, e, V, S, U, C, hi, h_a_b);   // enqueued, not awaited
}
RSLF_API_CATCH
