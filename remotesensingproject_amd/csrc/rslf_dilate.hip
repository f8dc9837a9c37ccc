// librslf_hip.so: the dilation along u (K16, k16_dilate.hpp) -- rslf_volume_dilate_u makes a new volume f times as wide from a
// resident one, rslf_planes_undilate_u brings result planes of the dilated frame back to the source grid (with a form on host
// pointers, which is a strided copy and touches no device), rslf_dilated_width is the width rule.  And what a fine-to-coarse
// level needs around a dilated sweep (K18, k18_level_dilate.hpp): rslf_planes_dilate_ranges_u takes the level's per-pixel
// ranges into the dilated frame (with a host form), rslf_planes_undilate_many_u brings a sweep's planes back in one launch.
// C-ABI: include/rslf_hip.h.  One device.
#include "rslf_internal.hpp"
#include "rslf_plan_dilate.hpp"
#include "rslf_plan_level_dilate.hpp"

#include "k16_dilate.hpp"
#include "k18_level_dilate.hpp"

using namespace rslf;

namespace {

int width_fault(plan::DilateArg a, int U, int factor, int kind)
{
    switch (a) {
    case plan::kDilateOk:
        return RSLF_OK;
    case plan::kDilateBadWidth:
        return fail(RSLF_ERR_INVALID_ARG, "U=%d: a row has at least one column", U);
    case plan::kDilateBadFactor:
        return fail(RSLF_ERR_INVALID_ARG, "factor=%d: an integer in 1..%d", factor, kDilateMaxFactor);
    case plan::kDilateBadKind:
        return fail(RSLF_ERR_INVALID_ARG, "kind=%d: RSLF_DILATE_LINEAR, RSLF_DILATE_CUBIC or RSLF_DILATE_LANCZOS3", kind);
    case plan::kDilateTooWide:
        return fail(RSLF_ERR_UNSUPPORTED, "U=%d dilated by %d does not fit a row", U, factor);
    }
    return fail(RSLF_ERR_INTERNAL, "unknown dilation fault");
}

template <int TAPS>
int launch_dilate(hipStream_t st, unsigned grid, int C, const DilateArgs& a)
{
    switch (C) {
    case 1:
        hipLaunchKernelGGL((k16_dilate_u<TAPS, 1>), dim3(grid), dim3(plan::kDilateBlock), 0, st, a);
        break;
    case 3:
        hipLaunchKernelGGL((k16_dilate_u<TAPS, 3>), dim3(grid), dim3(plan::kDilateBlock), 0, st, a);
        break;
    default:
        return fail(RSLF_ERR_INTERNAL, "no dilation kernel for %d channels", C);
    }
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

int check_undilate(const void* in, const void* out, int elem_bytes, int U_dilated, int factor, int* U)
{
    if (!in || !out)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (in == out)
        return fail(RSLF_ERR_INVALID_ARG, "the output plane is the input plane");
    if (elem_bytes != 1 && elem_bytes != 4)
        return fail(RSLF_ERR_INVALID_ARG, "elem_bytes=%d: planes of 1-byte or 4-byte elements", elem_bytes);
    if (!dilate_factor_ok(factor))
        return fail(RSLF_ERR_INVALID_ARG, "factor=%d: an integer in 1..%d", factor, kDilateMaxFactor);
    *U = plan::undilated_width(U_dilated, factor);
    if (!*U)
        return fail(RSLF_ERR_INVALID_ARG, "U_dilated=%d is not factor * (U - 1) + 1 for factor=%d", U_dilated, factor);
    return RSLF_OK;
}

}  // namespace

extern "C" int rslf_dilated_width(int U, int factor, int* U_out) RSLF_API_TRY
{
    if (!U_out)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument: U_out");
    return width_fault(plan::dilated_width(U, factor, U_out), U, factor, 0);
}
RSLF_API_CATCH

extern "C" int rslf_volume_dilate_u(rslf_ctx* ctx, const rslf_volume* src, int factor, int kind, rslf_volume** out) RSLF_API_TRY
{
    if (!out)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument: out");
    if (src && *out == src)   // (the caller's one handle of the source: left as it is)
        return fail(RSLF_ERR_INVALID_ARG, "out holds the source volume: the call would overwrite its handle");
    *out = nullptr;
    if (!ctx || !src)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    int U_out = 0;
    int rc = width_fault(plan::dilate_args(src->U, factor, kind, &U_out), src->U, factor, kind);
    if (rc)
        return rc;
    if (!src->filled)
        return fail(RSLF_ERR_INVALID_ARG, "the source volume has not been filled");
    if (src->device != ctx->device)
        return fail(RSLF_ERR_INVALID_ARG, "volume lives on device %d, the context on device %d", src->device, ctx->device);
    rslf_volume* vol = nullptr;
    rc = rslf_volume_create(ctx, src->V, src->S, U_out, src->C, &vol);   // its limits on a row are the dilated row's too
    if (rc)
        return rc;
    VolumePtr owner(vol);   // freed on every failure below
    DilateArgs a = {};
    a.src = src->base, a.dst = vol->base;
    a.row_in = src->pitch * src->C, a.row_out = vol->pitch * vol->C;
    a.tiles_per_row = (int)plan::dilate_tiles_per_row(vol->pitch, vol->C);
    a.tiles = plan::dilate_tiles((long long)src->V * src->S, vol->pitch, vol->C);
    a.U = src->U, a.U_out = U_out, a.f = factor;
    a.lo = src->min_value, a.hi = src->max_value;
    a.wt = dilate_weights(kind, factor);
    const unsigned grid = plan::dilate_grid(a.tiles);
    switch (dilate_taps(kind)) {
    case 2:
        rc = launch_dilate<2>(ctx->stream, grid, src->C, a);
        break;
    case 4:
        rc = launch_dilate<4>(ctx->stream, grid, src->C, a);
        break;
    default:
        rc = launch_dilate<6>(ctx->stream, grid, src->C, a);
        break;
    }
    if (rc)
        return rc;
    // nothing leaves [lo, hi] and the source's samples are all present (phase 0): the range is the source's, no reduction
    vol->min_value = src->min_value;
    vol->max_value = src->max_value;
    vol->filled = true;
    *out = owner.release();
    return RSLF_OK;   // enqueued, not awaited
}
RSLF_API_CATCH

extern "C" int rslf_planes_undilate_u(rslf_ctx* ctx, const void* d_in, int elem_bytes, size_t rows, int U_dilated, int factor,
                                      void* d_out) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    int U = 0;
    const int rc = check_undilate(d_in, d_out, elem_bytes, U_dilated, factor, &U);
    if (rc)
        return rc;
    if (!rows)
        return RSLF_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const dim3 grid(plan::undilate_grid_x(U), plan::undilate_grid_y(rows));
    if (elem_bytes == 1)
        hipLaunchKernelGGL((k16_undilate_u<uint8_t>), grid, dim3(plan::kDilateBlock), 0, ctx->stream, static_cast<const uint8_t*>(d_in),
                           static_cast<uint8_t*>(d_out), rows, U_dilated, U, factor);
    else
        hipLaunchKernelGGL((k16_undilate_u<uint32_t>), grid, dim3(plan::kDilateBlock), 0, ctx->stream, static_cast<const uint32_t*>(d_in),
                           static_cast<uint32_t*>(d_out), rows, U_dilated, U, factor);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;   // enqueued, not awaited
}
RSLF_API_CATCH

extern "C" int rslf_planes_undilate_u_host(const void* h_in, size_t in_row_stride_bytes, int elem_bytes, size_t rows, int U_dilated,
                                           int factor, void* h_out, size_t out_row_stride_bytes) RSLF_API_TRY
{
    int U = 0;
    const int rc = check_undilate(h_in, h_out, elem_bytes, U_dilated, factor, &U);
    if (rc)
        return rc;
    const size_t in_stride = in_row_stride_bytes ? in_row_stride_bytes : (size_t)U_dilated * elem_bytes;
    const size_t out_stride = out_row_stride_bytes ? out_row_stride_bytes : (size_t)U * elem_bytes;
    if (in_stride < (size_t)U_dilated * elem_bytes || out_stride < (size_t)U * elem_bytes)
        return fail(RSLF_ERR_INVALID_ARG, "a row stride is shorter than its row");
    for (size_t r = 0; r < rows; r++) {
        const char* in = static_cast<const char*>(h_in) + r * in_stride;
        char* o = static_cast<char*>(h_out) + r * out_stride;
        if (elem_bytes == 1)
            for (int u = 0; u < U; u++)
                o[u] = in[(size_t)u * factor];
        else
            for (int u = 0; u < U; u++)
                memcpy(o + (size_t)u * 4, in + (size_t)u * factor * 4, 4);
    }
    return RSLF_OK;
}
RSLF_API_CATCH

// ---- K18: a level's ranges into the dilated frame, a sweep's planes back out of it ------------------------------------

namespace {

int check_ranges(const void* dmin, const void* dmax, const void* out_min, const void* out_max, int U, int factor, int* U_out)
{
    if (!dmin || !dmax || !out_min || !out_max)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (out_min == dmin || out_min == dmax || out_max == dmin || out_max == dmax || out_min == out_max)
        return fail(RSLF_ERR_INVALID_ARG, "an output plane is an input plane or the other output plane");
    return width_fault(plan::dilated_width(U, factor, U_out), U, factor, 0);
}

}  // namespace

extern "C" int rslf_planes_dilate_ranges_u(rslf_ctx* ctx, const float* d_dmin, const float* d_dmax, size_t rows, int U, int factor,
                                           float* d_dmin_out, float* d_dmax_out) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    int U_out = 0;
    const int rc = check_ranges(d_dmin, d_dmax, d_dmin_out, d_dmax_out, U, factor, &U_out);
    if (rc)
        return rc;
    if (!rows)
        return RSLF_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const dim3 grid(plan::ranges_grid_x(U_out), plan::ranges_grid_y(rows));
    const int vec = plan::ranges_vector_stores(d_dmin_out, d_dmax_out) ? 1 : 0;
    hipLaunchKernelGGL(k18_dilate_ranges, grid, dim3(plan::kDilateBlock), 0, ctx->stream, d_dmin, d_dmax, rows, U, U_out, factor, vec,
                       d_dmin_out, d_dmax_out);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;   // enqueued, not awaited
}
RSLF_API_CATCH

extern "C" int rslf_planes_dilate_ranges_u_host(const float* h_dmin, const float* h_dmax, size_t in_row_stride_bytes, size_t rows, int U,
                                                int factor, float* h_dmin_out, float* h_dmax_out, size_t out_row_stride_bytes) RSLF_API_TRY
{
    int U_out = 0;
    const int rc = check_ranges(h_dmin, h_dmax, h_dmin_out, h_dmax_out, U, factor, &U_out);
    if (rc)
        return rc;
    const size_t in_stride = in_row_stride_bytes ? in_row_stride_bytes : (size_t)U * sizeof(float);
    const size_t out_stride = out_row_stride_bytes ? out_row_stride_bytes : (size_t)U_out * sizeof(float);
    if (in_stride < (size_t)U * sizeof(float) || out_stride < (size_t)U_out * sizeof(float))
        return fail(RSLF_ERR_INVALID_ARG, "a row stride is shorter than its row");
    if (in_stride % sizeof(float) || out_stride % sizeof(float))
        return fail(RSLF_ERR_INVALID_ARG, "a row stride is not a multiple of %zu bytes", sizeof(float));
    for (size_t r = 0; r < rows; r++) {
        const float* lo = reinterpret_cast<const float*>(reinterpret_cast<const char*>(h_dmin) + r * in_stride);
        const float* hi = reinterpret_cast<const float*>(reinterpret_cast<const char*>(h_dmax) + r * in_stride);
        float* olo = reinterpret_cast<float*>(reinterpret_cast<char*>(h_dmin_out) + r * out_stride);
        float* ohi = reinterpret_cast<float*>(reinterpret_cast<char*>(h_dmax_out) + r * out_stride);
        for (int j = 0; j < U_out; j++) {
            olo[j] = ranges_lower(lo, j, factor);
            ohi[j] = ranges_upper(hi, j, factor);
        }
    }
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_planes_undilate_many_u(rslf_ctx* ctx, const void* const* d_in, void* const* d_out, const int* elem_bytes,
                                           int n_planes, size_t rows, int U_dilated, int factor) RSLF_API_TRY
{
    if (!ctx || !d_in || !d_out || !elem_bytes)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (n_planes < 1 || n_planes > plan::kUndilateMany4 + plan::kUndilateMany1)
        return fail(RSLF_ERR_INVALID_ARG, "n_planes=%d: 1..%d planes", n_planes, plan::kUndilateMany4 + plan::kUndilateMany1);
    UndilateManyArgs a = {};
    int U = 0;
    for (int pass = 0; pass < 2; pass++)   // the 4-byte planes first, then the 1-byte ones
        for (int k = 0; k < n_planes; k++) {
            if (pass == 0) {
                if (int rc = check_undilate(d_in[k], d_out[k], elem_bytes[k], U_dilated, factor, &U))
                    return rc;
                for (int m = 0; m < n_planes; m++)
                    if (d_out[k] == d_in[m] || (m != k && d_out[k] == d_out[m]))
                        return fail(RSLF_ERR_INVALID_ARG, "output plane %d is an input plane or another output plane", k);
            }
            if ((elem_bytes[k] == 4) != (pass == 0))
                continue;
            const int at = a.n4 + a.n1;
            a.in[at] = d_in[k], a.out[at] = d_out[k];
            ++(pass == 0 ? a.n4 : a.n1);
        }
    if (!plan::undilate_many_counts_ok(a.n4, a.n1))
        return fail(RSLF_ERR_INVALID_ARG, "%d planes of 4-byte and %d of 1-byte elements: at most %d and %d", a.n4, a.n1,
                    plan::kUndilateMany4, plan::kUndilateMany1);
    if (!rows)
        return RSLF_OK;
    a.rows = rows, a.U_dilated = U_dilated, a.U = U, a.f = factor;
    HIP_TRY(hipSetDevice(ctx->device));
    const dim3 grid(plan::undilate_grid_x(U), plan::undilate_grid_y(rows), plan::undilate_many_grid_z(a.n4, a.n1));
    hipLaunchKernelGGL(k18_undilate_many, grid, dim3(plan::kDilateBlock), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;   // enqueued, not awaited
}
RSLF_API_CATCH
