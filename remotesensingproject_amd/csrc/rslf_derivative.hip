// librslf_hip.so: the derivative channels (K17, k17_derivative.hpp) -- rslf_volume_derivative_channels makes a new
// three-channel volume (x, |dx/du|, |dx/dv|) from a resident one-channel volume, rslf_derivative_channels_dense does the same
// to a dense raw level of the pyramid on device pointers (derivative_channels_raw: the level loop's own call).  C-ABI:
// include/rslf_hip.h.  One device.
#include "rslf_internal.hpp"
#include "rslf_plan_derivative.hpp"

#include "k17_derivative.hpp"

using namespace rslf;

namespace {

int launch_derivative(hipStream_t st, bool integer, const DerivativeArgs& a)
{
    const unsigned grid = plan::derivative_grid(a.tiles);
    if (integer)
        hipLaunchKernelGGL((k17_derivative_channels<true>), dim3(grid), dim3(plan::kDerivBlock), 0, st, a);
    else
        hipLaunchKernelGGL((k17_derivative_channels<false>), dim3(grid), dim3(plan::kDerivBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

int shape_fault(plan::DerivativeArg f, int V, int S, int U)
{
    switch (f) {
    case plan::kDerivOk:
        return RSLF_OK;
    case plan::kDerivBadShape:
        return fail(RSLF_ERR_INVALID_ARG, "bad dimensions V=%d S=%d U=%d", V, S, U);
    case plan::kDerivTooLarge:
        return fail(RSLF_ERR_UNSUPPORTED, "V=%d S=%d U=%d: a row of 3 * U floats and the V * S rows are indexed by int", V, S, U);
    }
    return fail(RSLF_ERR_INTERNAL, "unknown derivative fault");
}

}  // namespace

// The raw form, enqueued on the context's stream: d_in [V][S][U] floats (integer elements: integer values) -> d_out
// [V][S][U][3].  hi: the cap of float elements; an integer type's own otherwise.
int rslf::derivative_channels_raw(rslf_ctx* ctx, const float* d_in, Elem e, int V, int S, int U, float weight, float hi, float* d_out)
{
    DerivativeArgs a = {};
    a.src = d_in, a.dst = d_out, a.partial = nullptr;
    a.tiles_per_row = plan::derivative_tiles_per_row(U);
    a.tiles = (long long)V * S * a.tiles_per_row;
    a.V = V, a.S = S, a.U = U;
    a.row_in = U, a.pitch = 0;
    a.bases_aligned = ((uintptr_t)d_in % 16 == 0 && (uintptr_t)d_out % 16 == 0) ? 1 : 0;
    a.v_aligned = ((long long)S * U % 4 == 0) ? 1 : 0;
    a.h = derivative_half_weight(weight);
    a.hi = e == Elem::F32 ? hi : derivative_hi_int(elem_bytes(e));
    return launch_derivative(ctx->stream, e != Elem::F32, a);
}

extern "C" int rslf_derivative_channels_dense(rslf_ctx* ctx, const float* d_in_vsu, int elem, int V, int S, int U, float weight, float hi,
                                              float* d_out_vsu3) RSLF_API_TRY
{
    if (!ctx || !d_in_vsu || !d_out_vsu3)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if ((const float*)d_out_vsu3 == d_in_vsu)
        return fail(RSLF_ERR_INVALID_ARG, "the output level is the input level");
    Elem e;
    if (int rc = elem_of(elem, &e))
        return rc;
    if (!plan::derivative_weight_ok(weight))
        return fail(RSLF_ERR_INVALID_ARG, "weight=%g: a finite weight > 0", (double)weight);
    if (e == Elem::F32 && !plan::derivative_hi_ok(hi))
        return fail(RSLF_ERR_INVALID_ARG, "hi=%g: the cap of float elements is max(m, 0) of the source's maximum m", (double)hi);
    if (int rc = shape_fault(plan::derivative_shape(V, S, U), V, S, U))
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return derivative_channels_raw(ctx, d_in_vsu, e, V, S, U, weight, hi, d_out_vsu3);   // enqueued, not awaited
}
RSLF_API_CATCH

extern "C" int rslf_volume_derivative_channels(rslf_ctx* ctx, const rslf_volume* src, float weight, rslf_volume** out) RSLF_API_TRY
{
    if (!out)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument: out");
    if (src && *out == src)   // (the caller's one handle of the source: left as it is)
        return fail(RSLF_ERR_INVALID_ARG, "out holds the source volume: the call would overwrite its handle");
    *out = nullptr;
    if (!ctx || !src)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (!plan::derivative_weight_ok(weight))
        return fail(RSLF_ERR_INVALID_ARG, "weight=%g: a finite weight > 0", (double)weight);
    if (src->C != 1)
        return fail(RSLF_ERR_UNSUPPORTED, "C=%d: the derivative channels are built for a one-channel source (one channel and two features are three)", src->C);
    if (!src->filled)
        return fail(RSLF_ERR_INVALID_ARG, "the source volume has not been filled");
    if (src->device != ctx->device)
        return fail(RSLF_ERR_INVALID_ARG, "volume lives on device %d, the context on device %d", src->device, ctx->device);
    rslf_volume* vol = nullptr;
    int rc = rslf_volume_create(ctx, src->V, src->S, src->U, kDerivativeChannels, &vol);   // its limits on a row are the new row's
    if (rc)
        return rc;
    VolumePtr owner(vol);   // freed on every failure below
    DerivativeArgs a = {};
    a.src = src->base, a.dst = vol->base;
    a.tiles_per_row = plan::derivative_tiles_per_row(src->pitch);
    a.tiles = (long long)src->V * src->S * a.tiles_per_row;
    const unsigned grid = plan::derivative_grid(a.tiles);
    rc = range_partials(ctx, grid, &a.partial);
    if (rc)
        return rc;
    a.V = src->V, a.S = src->S, a.U = src->U;
    a.row_in = src->pitch, a.pitch = src->pitch;   // (vol->pitch is the same: the pitch is a function of U)
    a.bases_aligned = 1, a.v_aligned = 1;
    a.h = derivative_half_weight(weight);
    a.hi = derivative_hi_f32(src->max_value);
    rc = launch_derivative(ctx->stream, false, a);
    if (rc)
        return rc;
    // the new slab's own range, as an upload of it would find it: the minimum can be a feature's (0 where the source is
    // positive), the maximum is the source's by the cap.  The two floats are waited for, as the uploads wait for theirs.
    rc = volume_range_from_partials(vol, (int)grid);
    if (rc)
        return rc;
    *out = owner.release();
    return RSLF_OK;
}
RSLF_API_CATCH
