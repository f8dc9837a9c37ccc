// librslf_hip.so, unit 1 of 9: errors, contexts, volumes, host upload / device pack (K0).
// C-ABI: include/rslf_hip.h.  No OpenCV, no torch, no CPU compute path.
#include "rslf_internal.hpp"

#include <algorithm>
#include <cmath>

#include "k0_pack.hpp"

using namespace rslf;

// ---- errors ---------------------------------------------------------------

namespace rslf {

char* last_error_buffer()
{
    static thread_local char g_err[512] = "";
    return g_err;
}

static std::atomic<int> g_inject[kInjectSites];

bool inject_hit(InjectSite site)
{
    std::atomic<int>& c = g_inject[site];
    int v = c.load(std::memory_order_relaxed);
    while (v > 0)
        if (c.compare_exchange_weak(v, v - 1, std::memory_order_relaxed))
            return true;
    return false;
}

}  // namespace rslf

extern "C" int rslf_debug_inject(const char* site, int count) RSLF_API_TRY
{
    if (!site || count < 0)
        return fail(RSLF_ERR_INVALID_ARG, "rslf_debug_inject: bad argument");
    static const char* const names[kInjectSites] = {"worker", "thread_create", "alloc", "sweep"};
    for (int i = 0; i < kInjectSites; i++)
        if (strcmp(site, names[i]) == 0) {
            g_inject[i].store(count, std::memory_order_relaxed);
            return RSLF_OK;
        }
    return fail(RSLF_ERR_INVALID_ARG, "rslf_debug_inject: unknown site %s", site);
}
RSLF_API_CATCH

// Pixel lists and the raw-disparity plane of V x U pixels, per-scanline counts and row bases of V scanlines
int rslf::ensure_plane_scratch(rslf_ctx* ctx, int V, int U)
{
    Scratch& sc = ctx->scratch;
    const size_t n = (size_t)V * U;
    HIP_TRY(hip_err(sc.list.reserve(n * sizeof(int))));
    HIP_TRY(hip_err(sc.depth_tmp.reserve(n * sizeof(float))));
    HIP_TRY(hip_err(sc.count.reserve((size_t)V * sizeof(int))));
    HIP_TRY(hip_err(sc.rowbase.reserve((size_t)V * sizeof(int))));
    return RSLF_OK;
}

// Records and tickets of grouped scan launches (k2_scan.hpp): grow-only, so a context allocates them once.
// tickets_fresh (nullable): new tickets were made, and their zeros are queued on the context's stream.
int rslf::ensure_group_scratch(rslf_ctx* ctx, size_t recs, size_t tiles, bool* tickets_fresh)
{
    Scratch& sc = ctx->scratch;
    HIP_TRY(hip_err(sc.scan_partial.reserve(recs * plan::kPartialRecordBytes)));
    const Reserved t = sc.scan_ticket.reserve(tiles * sizeof(int));
    HIP_TRY(hip_err(t));
    if (t.fresh)   // the kernels leave it at zero
        HIP_TRY(hipMemsetAsync(sc.scan_ticket.get(), 0, sc.scan_ticket.capacity(), ctx->stream));
    if (tickets_fresh)
        *tickets_fresh = t.fresh;
    return RSLF_OK;
}

// ---- misc -----------------------------------------------------------------

extern "C" int rslf_abi_version(void) RSLF_API_TRY
{
    return RSLF_ABI_VERSION;
}
RSLF_API_CATCH

extern "C" const char* rslf_status_string(int status)
{
    switch (status) {
    case RSLF_OK: return "ok";
    case RSLF_ERR_INVALID_ARG: return "invalid argument";
    case RSLF_ERR_UNSUPPORTED: return "unsupported configuration";
    case RSLF_ERR_HIP: return "HIP runtime error";
    case RSLF_ERR_NO_DEVICE: return "no gfx950 device";
    case RSLF_ERR_ALLOC: return "allocation failed";
    case RSLF_ERR_INTERNAL: return "internal error (an exception was stopped at the C boundary)";
    default: return "unknown status";
    }
}

extern "C" const char* rslf_last_error(void) { return last_error_buffer(); }

extern "C" int rslf_device_count(void) RSLF_API_TRY
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}
RSLF_API_CATCH

extern "C" void rslf_default_params(rslf_params* p)
{
    if (!p)
        return;
    // include/rslf_depth_computation_core.hpp:16-31, :74-99
    p->edge_score_threshold = (float)0.02;
    p->line_score_threshold = (float)0.02;
    p->disp_score_threshold = (float)0.01;
    p->raw_score_threshold = (float)0;
    p->mean_shift_max_iter = (float)10;
    p->edge_confidence_filter_size = 9;
    p->edge_confidence_opening_type = 2;
    p->edge_confidence_opening_size = 1;
    p->median_filter_size = 5;
    p->median_filter_epsilon = (float)0.1;
    p->propagation_epsilon = (float)0.1;
    p->slope_factor = (float)1.0;
    p->cut_shadows = 1;
    p->shadow_level = (float)(0.05 * 1.73205080757);
    p->kernel_bandwidth = (float)0.2;
    p->interpolation = RSLF_INTERP_LINEAR;   // core.hpp:76
    p->use_disp_confidence_score = 0;        // core.hpp:35: commented out in the reference
}

ScanConsts rslf::make_scan_consts(const rslf_params* p)
{
    ScanConsts k;
    k.slope = p->slope_factor;
    const float h = p->kernel_bandwidth;
    const float hh = h * h;
    k.inv_h2 = (float)(1.0 / (double)hh);   // include/rslf_kernels.hpp:43
    k.k1 = 3.0f * k.inv_h2;                 // src/rslf_kernels.cpp:21
    k.raw_thr = p->raw_score_threshold;
    k.n_iter = plan::mean_shift_passes(p->mean_shift_max_iter);   // core.hpp:584, float bound
    k.interp = p->interpolation;
    return k;
}

int rslf::check_params(const rslf_params* p)
{
    if (!p)
        return fail(RSLF_ERR_INVALID_ARG, "params is NULL");
    if (p->edge_confidence_opening_size > 31)
        return fail(RSLF_ERR_UNSUPPORTED, "edge_confidence_opening_size=%d: structuring elements up to 31 x 31", p->edge_confidence_opening_size);
    if (p->edge_confidence_opening_size > 1 && (p->edge_confidence_opening_type < 0 || p->edge_confidence_opening_type > 2))
        return fail(RSLF_ERR_INVALID_ARG, "edge_confidence_opening_type=%d is not cv::MORPH_RECT (0), MORPH_CROSS (1) or MORPH_ELLIPSE (2)",
                    p->edge_confidence_opening_type);
    if (p->edge_confidence_filter_size < 1 || (p->edge_confidence_filter_size & 1) == 0)
        return fail(RSLF_ERR_INVALID_ARG, "edge_confidence_filter_size must be odd and >= 1");
    // any window the reference runs: width = (size - 1) / 2 (core.hpp:686), so even sizes and 0 are fine; a negative size
    // has no window at all (the reference then reads an empty vector, core.hpp:713-714)
    if (p->median_filter_size < 0 || p->median_filter_size > plan::kMedianMaxSize)
        return fail(RSLF_ERR_INVALID_ARG, "median_filter_size=%d: must be in [0, %d]", p->median_filter_size, plan::kMedianMaxSize);
    if (!(p->kernel_bandwidth > 0.0f))
        return fail(RSLF_ERR_INVALID_ARG, "kernel_bandwidth must be > 0");
    if (!(p->mean_shift_max_iter > 0.0f))
        return fail(RSLF_ERR_INVALID_ARG, "mean_shift_max_iter must be > 0");
    if (p->interpolation < RSLF_INTERP_LINEAR || p->interpolation > RSLF_INTERP_NEAREST_AS_BUILT)
        return fail(RSLF_ERR_INVALID_ARG, "interpolation=%d is not one of RSLF_INTERP_*", p->interpolation);
    return RSLF_OK;
}

// ---- context --------------------------------------------------------------

extern "C" int rslf_ctx_create(int device, rslf_ctx** out) RSLF_API_TRY
{
    if (!out)
        return fail(RSLF_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(RSLF_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n)
        return fail(RSLF_ERR_INVALID_ARG, "device %d out of range (0..%d)", device, n - 1);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RSLF_ERR_NO_DEVICE, "device %d is %s; this library holds gfx950 code objects only", device, prop.gcnArchName);
    HIP_TRY(hipSetDevice(device));
    rslf_ctx* ctx = new (std::nothrow) rslf_ctx();
    if (!ctx)
        return fail(RSLF_ERR_ALLOC, "out of host memory");
    ctx->device = device;
    (void)hipDeviceGetAttribute(&ctx->num_cus, hipDeviceAttributeMultiprocessorCount, device);
    hipError_t e = hip_err(ctx->scratch.total.reserve(2 * sizeof(unsigned long long)));   // Scratch::pixel_total, packed_len
    if (e == hipSuccess)
        e = hip_err(ctx->scratch.minmax.reserve(2 * sizeof(float)));
    if (e == hipSuccess)
        e = hipEventCreate(&ctx->ev0);
    if (e == hipSuccess)
        e = hipEventCreate(&ctx->ev1);
    if (e != hipSuccess) {
        (void)rslf_ctx_destroy(ctx);   // whatever of total / minmax / the events was made goes with it
        return fail(RSLF_ERR_HIP, "context setup failed: %s", hipGetErrorString(e));
    }
    *out = ctx;
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_ctx_destroy(rslf_ctx* ctx) RSLF_API_TRY
{
    if (!ctx)
        return RSLF_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (hipEvent_t e : ctx->ev_pool)
        (void)hipEventDestroy(e);
    if (ctx->ev0)
        (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1)
        (void)hipEventDestroy(ctx->ev1);
    delete ctx;   // every buffer of ctx->scratch is freed by its destructor
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_ctx_set_stream(rslf_ctx* ctx, void* hip_stream) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "ctx is NULL");
    ctx->stream = (hipStream_t)hip_stream;
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_ctx_set_debug(rslf_ctx* ctx, const char* key, int value) RSLF_API_TRY
{
    if (!ctx || !key)
        return fail(RSLF_ERR_INVALID_ARG, "ctx/key is NULL");
    if (strcmp(key, "force_scan") == 0 && value >= 0 && value <= 2)
        ctx->force_scan = value;
    else if (strcmp(key, "force_groups") == 0 && value >= 0 && value <= 64)
        ctx->force_groups = value;
    else if (strcmp(key, "force_packed") == 0 && value >= -1 && value <= 1)
        ctx->force_packed = value;
    else if (strcmp(key, "px") == 0 && value >= -1 && value <= 1)
        ctx->px_mode = value;
    else if (strcmp(key, "stream_share") == 0 && value >= 0 && value <= 2)
        ctx->stream_share = value;
    else if (strcmp(key, "row_split") == 0 && value >= 0 && value <= 65536)
        ctx->row_split = value;
    else if (strcmp(key, "tap_table") == 0 && (value == 0 || value == 1))
        ctx->tap_table = value;
    else if (strcmp(key, "scalar_taps") == 0 && (value == 0 || value == 1))
        ctx->scalar_taps = value;
    else if (strcmp(key, "claim_skip") == 0 && (value == 0 || value == 1))
        ctx->claim_skip = value;
    else if (strcmp(key, "subgrid_list") == 0 && (value == 0 || value == 1))
        ctx->subgrid_list = value;
    else if (strcmp(key, "peaks_list") == 0 && (value == 0 || value == 1))
        ctx->peaks_list = value;
    else if (strcmp(key, "consistency_order") == 0 && value >= 0 && value <= 2)
        ctx->consistency_order = value;
    else if (strcmp(key, "time_all") == 0 && (value == 0 || value == 1)) {
        ctx->time_all = value;
        ctx->ev_used = 0;
    } else if (strcmp(key, "stream_groups") == 0 && value >= 0 && value <= 64)
        ctx->stream_groups = value;
    else if (strcmp(key, "stream_lds_kib") == 0 && value >= 16 && value <= 152) {
        ctx->stream_lds_bytes = (size_t)value << 10;
    } else if (strcmp(key, "staging_kib") == 0 && value >= 0 && value <= 262144)
        ctx->staging_kib = value;
    else
        return fail(RSLF_ERR_INVALID_ARG, "rslf_ctx_set_debug: unknown key or value out of range: %s = %d", key, value);
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_ctx_synchronize(rslf_ctx* ctx) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RSLF_OK;
}
RSLF_API_CATCH

// ---- volume ---------------------------------------------------------------

extern "C" int rslf_volume_create(rslf_ctx* ctx, int V, int S, int U, int C, rslf_volume** out) RSLF_API_TRY
{
    if (!ctx || !out)
        return fail(RSLF_ERR_INVALID_ARG, "ctx/out is NULL");
    *out = nullptr;
    if (V < 1 || S < 1 || U < 1)
        return fail(RSLF_ERR_INVALID_ARG, "bad dimensions V=%d S=%d U=%d", V, S, U);
    if (C != 1 && C != 3)
        return fail(RSLF_ERR_UNSUPPORTED, "C=%d: the reference instantiates float and cv::Vec3f only (dc.hpp:149-154)", C);
    if (V > 65535 || S > 65535)
        return fail(RSLF_ERR_UNSUPPORTED, "V=%d / S=%d: the per-scanline kernels index scanlines and views with grid.y / grid.z "
                                          "(at most 65535)", V, S);
    if ((long long)S * C * (((long long)U + 1 + 63) / 64 * 64) > ((long long)1 << 29))
        return fail(RSLF_ERR_UNSUPPORTED, "one EPI (S*pitch*C floats) must stay below 2 GiB: the scan addresses it with 32-bit byte offsets");
    HIP_TRY(hipSetDevice(ctx->device));
    rslf_volume* vol = new (std::nothrow) rslf_volume();
    if (!vol)
        return fail(RSLF_ERR_ALLOC, "out of host memory");
    vol->ctx = ctx;
    vol->device = ctx->device;
    vol->V = V;
    vol->S = S;
    vol->U = U;
    vol->C = C;
    vol->pitch = plan::volume_pitch(U);   // pixels per row, > U: the second lerp tap of u = U-1 lands on zeros
    vol->bytes = plan::volume_bytes(V, S, U, C);
    hipError_t e = hipMalloc(&vol->base, vol->bytes);
    if (e != hipSuccess) {
        delete vol;
        return fail(RSLF_ERR_ALLOC, "hipMalloc(%zu) for the volume failed: %s", vol->bytes, hipGetErrorString(e));
    }
    *out = vol;
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_volume_destroy(rslf_volume* vol) RSLF_API_TRY
{
    if (!vol)
        return RSLF_OK;
    // hipFree waits for the device's outstanding work, so the slab outlives every launch that reads it; the
    // context is not touched (it may already be gone -- contexts and volumes can be destroyed in either order)
    (void)hipSetDevice(vol->device);
    (void)hipFree(vol->base);
    delete vol;
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_volume_describe(const rslf_volume* vol, rslf_volume_desc* out) RSLF_API_TRY
{
    if (!vol || !out)
        return fail(RSLF_ERR_INVALID_ARG, "vol/out is NULL");
    out->V = vol->V;
    out->S = vol->S;
    out->U = vol->U;
    out->C = vol->C;
    out->pitch = vol->pitch;
    out->d_base = vol->base;
    out->bytes = vol->bytes;
    out->min_value = vol->min_value;
    out->max_value = vol->max_value;
    return RSLF_OK;
}
RSLF_API_CATCH

static int ensure_partial(rslf_ctx* ctx, size_t rows)
{
    HIP_TRY(hip_err(ctx->scratch.partial.reserve(rows * 2 * sizeof(float))));
    return RSLF_OK;
}

int rslf::ensure_staging(rslf_ctx* ctx, size_t bytes)
{
    HIP_TRY(hip_err(ctx->scratch.staging.reserve(bytes)));
    return RSLF_OK;
}

// Shared buffer `which` (SharedBuf in rslf_internal.hpp: who shares it and why that is safe), at least `bytes` large.
// Growing it frees the old buffer, which waits for the device; after the first call of a given size nothing is allocated
// any more.
int rslf::helper_scratch(rslf_ctx* ctx, SharedBuf which, size_t bytes, void** out)
{
    DeviceBuf& b = ctx->scratch.shared[which];
    HIP_TRY(hip_err(b.reserve(bytes)));
    *out = b.get();
    return RSLF_OK;
}

__global__ void k_init_minmax(float* minmax)
{
    minmax[0] = INFINITY;
    minmax[1] = -INFINITY;
}

static int minmax_begin(rslf_ctx* ctx)
{
    hipLaunchKernelGGL(k_init_minmax, dim3(1), dim3(1), 0, ctx->stream, ctx->scratch.minmax.as<float>());
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

static int minmax_end(rslf_volume* vol)
{
    rslf_ctx* ctx = vol->ctx;
    float mm[2];
    HIP_TRY(hipMemcpyAsync(mm, ctx->scratch.minmax.get(), sizeof(mm), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    vol->min_value = mm[0];
    vol->max_value = mm[1];
    vol->filled = true;
    return RSLF_OK;
}

// The range of a volume whose slab a kernel of another unit wrote (K17): that kernel leaves n (min, max) pairs, as K0's
// rows do, in the buffer range_partials hands out; volume_range_from_partials folds them as the uploads fold theirs, waits
// for the two floats and marks the volume filled.
int rslf::range_partials(rslf_ctx* ctx, size_t n, float** out)
{
    const int rc = ensure_partial(ctx, n);
    if (!rc)
        *out = ctx->scratch.partial.as<float>();
    return rc;
}

int rslf::volume_range_from_partials(rslf_volume* vol, int n)
{
    rslf_ctx* ctx = vol->ctx;
    const int rc = minmax_begin(ctx);
    if (rc)
        return rc;
    hipLaunchKernelGGL(k0_minmax_final, dim3(1), dim3(256), 0, ctx->stream, ctx->scratch.partial.as<float>(), n,
                       ctx->scratch.minmax.as<float>());
    HIP_TRY(hipGetLastError());
    return minmax_end(vol);
}

// Pack rows [V0, V0+Vn) from a device buffer holding just those rows.
template <typename SrcT>
static int pack_chunk(rslf_volume* vol, const SrcT* d_src, int V0, int Vn, bool image_major, float scale)
{
    rslf_ctx* ctx = vol->ctx;
    const size_t rows = (size_t)Vn * vol->S;
    int rc = ensure_partial(ctx, rows);
    if (rc)
        return rc;
    if (image_major)
        hipLaunchKernelGGL((k0_pack<SrcT, true>), dim3((unsigned)rows), dim3(256), 0, ctx->stream, d_src, vol->base, V0, Vn, Vn,
                           vol->S, vol->U, vol->C, vol->pitch, scale, ctx->scratch.partial.as<float>());
    else
        hipLaunchKernelGGL((k0_pack<SrcT, false>), dim3((unsigned)rows), dim3(256), 0, ctx->stream, d_src, vol->base, V0, Vn, Vn,
                           vol->S, vol->U, vol->C, vol->pitch, scale, ctx->scratch.partial.as<float>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k0_minmax_final, dim3(1), dim3(256), 0, ctx->stream, ctx->scratch.partial.as<float>(), (int)rows,
                       ctx->scratch.minmax.as<float>());
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

// Bytes of device staging one pass of a chunked host upload may take: plan::kStagingBudget, or the "staging_kib" hook.
static size_t staging_budget(const rslf_ctx* ctx)
{
    return ctx->staging_kib > 0 ? (size_t)ctx->staging_kib << 10 : plan::kStagingBudget;
}

// Host upload in scanline chunks through a bounded device staging buffer.
template <typename SrcT>
int rslf::upload_host(rslf_volume* vol, const SrcT* const* h_ptrs, size_t row_stride_bytes, bool image_major, float scale)
{
    rslf_ctx* ctx = vol->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t row_bytes = (size_t)vol->U * vol->C * sizeof(SrcT);
    if (row_stride_bytes == 0)
        row_stride_bytes = row_bytes;
    if (row_stride_bytes < row_bytes)
        return fail(RSLF_ERR_INVALID_ARG, "row_stride_bytes %zu < row size %zu", row_stride_bytes, row_bytes);
    const size_t epi_bytes = row_bytes * vol->S;
    const int chunk = plan::staging_chunk_rows(epi_bytes, vol->V, staging_budget(ctx));
    int rc = ensure_staging(ctx, (size_t)chunk * epi_bytes);
    if (rc)
        return rc;
    char* const staging = ctx->scratch.staging.as<char>();
    rc = minmax_begin(ctx);
    if (rc)
        return rc;
    for (int v0 = 0; v0 < vol->V; v0 += chunk) {
        const int vn = std::min(chunk, vol->V - v0);
        if (!image_major) {
            // h_ptrs[v] -> S rows; staging [vn][S][U*C]
            for (int i = 0; i < vn; i++)
                if (!h_ptrs[v0 + i])
                    return fail(RSLF_ERR_INVALID_ARG, "h_epis[%d] is NULL", v0 + i);
            // Dense rows (the usual cv::Mat): an EPI is one run of bytes, and EPIs that follow one another in host memory
            // (a stacked array) are one run together -- plain 1-D copies, which move pageable memory at the link's rate
            // (57 GB/s measured, tools/probe_h2d.py) where the 2-D form with its 8 KB rows reached about 10.
            for (int i = 0; i < vn;) {
                if (row_stride_bytes != row_bytes) {
                    HIP_TRY(hipMemcpy2DAsync(staging + (size_t)i * epi_bytes, row_bytes, h_ptrs[v0 + i], row_stride_bytes,
                                             row_bytes, vol->S, hipMemcpyHostToDevice, ctx->stream));
                    i++;
                    continue;
                }
                int n = 1;
                while (i + n < vn && (const char*)h_ptrs[v0 + i + n] == (const char*)h_ptrs[v0 + i] + (size_t)n * epi_bytes)
                    n++;
                HIP_TRY(hipMemcpyAsync(staging + (size_t)i * epi_bytes, h_ptrs[v0 + i], (size_t)n * epi_bytes,
                                       hipMemcpyHostToDevice, ctx->stream));
                i += n;
            }
        } else {
            // h_ptrs[s] -> V rows; staging [S][vn][U*C]
            for (int s = 0; s < vol->S; s++) {
                if (!h_ptrs[s])
                    return fail(RSLF_ERR_INVALID_ARG, "h_imgs[%d] is NULL", s);
                if (row_stride_bytes == row_bytes)   // dense rows: one run of bytes (see above)
                    HIP_TRY(hipMemcpyAsync(staging + (size_t)s * vn * row_bytes, (const char*)h_ptrs[s] + (size_t)v0 * row_bytes,
                                           (size_t)vn * row_bytes, hipMemcpyHostToDevice, ctx->stream));
                else
                    HIP_TRY(hipMemcpy2DAsync(staging + (size_t)s * vn * row_bytes, row_bytes,
                                             (const char*)h_ptrs[s] + (size_t)v0 * row_stride_bytes, row_stride_bytes, row_bytes, vn,
                                             hipMemcpyHostToDevice, ctx->stream));
            }
        }
        rc = pack_chunk<SrcT>(vol, (const SrcT*)staging, v0, vn, image_major, scale);
        if (rc)
            return rc;
        // the staging buffer is reused by the next chunk
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return minmax_end(vol);
}

// Image-major upload with build_epis_from_imgs' transpose / rotate_180 options: n_imgs images of V rows x cols.
template <typename SrcT>
static int upload_images_xf(rslf_volume* vol, const SrcT* const* h_imgs, size_t row_stride_bytes, float scale, int transpose,
                            int rotate_180)
{
    rslf_ctx* ctx = vol->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const int n_imgs = transpose ? vol->U : vol->S;   // the slab holds E^T when transposed
    const int cols = transpose ? vol->S : vol->U;
    const size_t row_bytes = (size_t)cols * vol->C * sizeof(SrcT);
    if (row_stride_bytes == 0)
        row_stride_bytes = row_bytes;
    if (row_stride_bytes < row_bytes)
        return fail(RSLF_ERR_INVALID_ARG, "row_stride_bytes %zu < row size %zu", row_stride_bytes, row_bytes);
    const size_t epi_bytes = row_bytes * n_imgs;
    const int chunk = plan::staging_chunk_rows(epi_bytes, vol->V, staging_budget(ctx));
    int rc = ensure_staging(ctx, (size_t)chunk * epi_bytes);
    if (rc)
        return rc;
    char* const staging = ctx->scratch.staging.as<char>();
    rc = minmax_begin(ctx);
    if (rc)
        return rc;
    for (int v0 = 0; v0 < vol->V; v0 += chunk) {
        const int vn = std::min(chunk, vol->V - v0);
        for (int i = 0; i < n_imgs; i++) {   // staging [n_imgs][vn][cols*C]
            if (!h_imgs[i])
                return fail(RSLF_ERR_INVALID_ARG, "h_imgs[%d] is NULL", i);
            if (row_stride_bytes == row_bytes)
                HIP_TRY(hipMemcpyAsync(staging + (size_t)i * vn * row_bytes, (const char*)h_imgs[i] + (size_t)v0 * row_bytes,
                                       (size_t)vn * row_bytes, hipMemcpyHostToDevice, ctx->stream));
            else
                HIP_TRY(hipMemcpy2DAsync(staging + (size_t)i * vn * row_bytes, row_bytes,
                                         (const char*)h_imgs[i] + (size_t)v0 * row_stride_bytes, row_stride_bytes, row_bytes, vn,
                                         hipMemcpyHostToDevice, ctx->stream));
        }
        const size_t rows = (size_t)vn * vol->S;
        rc = ensure_partial(ctx, rows);
        if (rc)
            return rc;
        float* const partial = ctx->scratch.partial.as<float>();
        hipLaunchKernelGGL((k0_pack_images_xf<SrcT>), dim3((unsigned)rows), dim3(256), 0, ctx->stream, (const SrcT*)staging,
                           vol->base, v0, vn, n_imgs, cols, vol->S, vol->U, vol->C, vol->pitch, scale, transpose, rotate_180,
                           partial);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k0_minmax_final, dim3(1), dim3(256), 0, ctx->stream, partial, (int)rows, ctx->scratch.minmax.as<float>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));   // the staging buffer is reused by the next chunk
    }
    return minmax_end(vol);
}

// dc.hpp:442-460: epi_scale_factor = max over every value of every EPI
template <>
float rslf::host_max<float>(const float* const* h_ptrs, int n_ptrs, int rows, size_t row_stride_bytes, size_t row_elems, float start)
{
    float m = start;
    for (int i = 0; i < n_ptrs; i++) {
        for (int r = 0; r < rows; r++) {
            const float* p = (const float*)((const char*)h_ptrs[i] + (size_t)r * row_stride_bytes);
            for (size_t k = 0; k < row_elems; k++)
                if (p[k] > m)
                    m = p[k];
        }
    }
    return m;
}
// ushort: the max taken in integers (a vectorised pass), then widened -- float(max x) == max float(x), the conversion
// being exact and monotone
template <>
float rslf::host_max<uint16_t>(const uint16_t* const* h_ptrs, int n_ptrs, int rows, size_t row_stride_bytes, size_t row_elems,
                               float start)
{
    uint16_t mx = 0;
    for (int i = 0; i < n_ptrs; i++) {
        for (int r = 0; r < rows; r++) {
            const uint16_t* p = (const uint16_t*)((const char*)h_ptrs[i] + (size_t)r * row_stride_bytes);
            uint16_t rm = 0;
            for (size_t k = 0; k < row_elems; k++)
                rm = p[k] > rm ? p[k] : rm;
            mx = rm > mx ? rm : mx;
        }
    }
    const bool any = n_ptrs > 0 && rows > 0 && row_elems > 0;
    return any && (float)mx > start ? (float)mx : start;
}

float rslf::resolve_scale_factor(Elem e, const void* const* h_ptrs, int n_ptrs, int rows, size_t row_stride_bytes, size_t row_elems,
                                 float epi_scale_factor, bool parallel)
{
    if (e == Elem::U8)
        return 255.0f;   // dc.hpp:470
    if (!(epi_scale_factor < 0))
        return epi_scale_factor;
    if (e == Elem::F32)
        return parallel ? host_max_parallel((const float* const*)h_ptrs, n_ptrs, rows, row_stride_bytes, row_elems, epi_scale_factor)
                        : host_max((const float* const*)h_ptrs, n_ptrs, rows, row_stride_bytes, row_elems, epi_scale_factor);
    return parallel ? host_max_parallel((const uint16_t* const*)h_ptrs, n_ptrs, rows, row_stride_bytes, row_elems, epi_scale_factor)
                    : host_max((const uint16_t* const*)h_ptrs, n_ptrs, rows, row_stride_bytes, row_elems, epi_scale_factor);
}

int rslf::upload_host_elem(rslf_volume* vol, Elem e, const void* const* h_ptrs, size_t row_stride_bytes, bool image_major, float scale)
{
    switch (e) {
    case Elem::U8:
        return upload_host<uint8_t>(vol, (const uint8_t* const*)h_ptrs, row_stride_bytes, image_major, scale);
    case Elem::U16:
        return upload_host<uint16_t>(vol, (const uint16_t* const*)h_ptrs, row_stride_bytes, image_major, scale);
    default:
        return upload_host<float>(vol, (const float* const*)h_ptrs, row_stride_bytes, image_major, scale);
    }
}

// The three host uploads for one element type.  n_ptrs pointers of `rows` rows each, of row_elems values: EPIs
// (V x S), images (S x V), or the images of the transposing form.  The scale rule is resolve_scale_factor's.
static int upload_epis_elem(rslf_volume* vol, Elem e, const void* const* h_epis, size_t row_stride_bytes, float epi_scale_factor,
                            float* scale_used)
{
    if (!vol || !h_epis)
        return fail(RSLF_ERR_INVALID_ARG, "vol/h_epis is NULL");
    const size_t row_elems = (size_t)vol->U * vol->C;
    const size_t row_bytes = row_elems * elem_bytes(e);
    const size_t stride = row_stride_bytes ? row_stride_bytes : row_bytes;
    if (stride < row_bytes)
        return fail(RSLF_ERR_INVALID_ARG, "row_stride_bytes %zu < row size %zu", stride, row_bytes);
    for (int v = 0; v < vol->V; v++)
        if (!h_epis[v])
            return fail(RSLF_ERR_INVALID_ARG, "h_epis[%d] is NULL", v);
    epi_scale_factor = resolve_scale_factor(e, h_epis, vol->V, vol->S, stride, row_elems, epi_scale_factor, false);
    if (scale_used)
        *scale_used = epi_scale_factor;
    return upload_host_elem(vol, e, h_epis, stride, false, scale_of(epi_scale_factor));
}

static int upload_images_elem(rslf_volume* vol, Elem e, const void* const* h_imgs, size_t row_stride_bytes, float epi_scale_factor,
                              float* scale_used)
{
    if (!vol || !h_imgs)
        return fail(RSLF_ERR_INVALID_ARG, "vol/h_imgs is NULL");
    const size_t row_elems = (size_t)vol->U * vol->C;
    const size_t row_bytes = row_elems * elem_bytes(e);
    const size_t stride = row_stride_bytes ? row_stride_bytes : row_bytes;
    if (stride < row_bytes)
        return fail(RSLF_ERR_INVALID_ARG, "row_stride_bytes %zu < row size %zu", stride, row_bytes);
    for (int s = 0; s < vol->S; s++)
        if (!h_imgs[s])
            return fail(RSLF_ERR_INVALID_ARG, "h_imgs[%d] is NULL", s);
    epi_scale_factor = resolve_scale_factor(e, h_imgs, vol->S, vol->V, stride, row_elems, epi_scale_factor, false);
    if (scale_used)
        *scale_used = epi_scale_factor;
    return upload_host_elem(vol, e, h_imgs, stride, true, scale_of(epi_scale_factor));
}

static int upload_images_xf_elem(rslf_volume* vol, Elem e, const void* const* h_imgs, size_t row_stride_bytes, float epi_scale_factor,
                                 float* scale_used, int transpose, int rotate_180)
{
    if (!vol || !h_imgs)
        return fail(RSLF_ERR_INVALID_ARG, "vol/h_imgs is NULL");
    const int n_imgs = transpose ? vol->U : vol->S;
    const size_t row_elems = (size_t)(transpose ? vol->S : vol->U) * vol->C;
    const size_t row_bytes = row_elems * elem_bytes(e);
    const size_t stride = row_stride_bytes ? row_stride_bytes : row_bytes;
    if (stride < row_bytes)
        return fail(RSLF_ERR_INVALID_ARG, "row_stride_bytes %zu < row size %zu", stride, row_bytes);
    for (int i = 0; i < n_imgs; i++)
        if (!h_imgs[i])
            return fail(RSLF_ERR_INVALID_ARG, "h_imgs[%d] is NULL", i);
    epi_scale_factor = resolve_scale_factor(e, h_imgs, n_imgs, vol->V, stride, row_elems, epi_scale_factor, false);
    if (scale_used)
        *scale_used = epi_scale_factor;
    const float scale = scale_of(epi_scale_factor);
    switch (e) {
    case Elem::U8:
        return upload_images_xf<uint8_t>(vol, (const uint8_t* const*)h_imgs, stride, scale, transpose != 0, rotate_180 != 0);
    case Elem::U16:
        return upload_images_xf<uint16_t>(vol, (const uint16_t* const*)h_imgs, stride, scale, transpose != 0, rotate_180 != 0);
    default:
        return upload_images_xf<float>(vol, (const float* const*)h_imgs, stride, scale, transpose != 0, rotate_180 != 0);
    }
}

extern "C" int rslf_volume_upload_epis_f32(rslf_volume* vol, const float* const* h_epis, size_t row_stride_bytes,
                                           float epi_scale_factor, float* scale_used) RSLF_API_TRY
{
    return upload_epis_elem(vol, Elem::F32, (const void* const*)h_epis, row_stride_bytes, epi_scale_factor, scale_used);
}
RSLF_API_CATCH

extern "C" int rslf_volume_upload_epis_u8(rslf_volume* vol, const uint8_t* const* h_epis, size_t row_stride_bytes) RSLF_API_TRY
{
    return upload_epis_elem(vol, Elem::U8, (const void* const*)h_epis, row_stride_bytes, -1.0f, nullptr);
}
RSLF_API_CATCH

extern "C" int rslf_volume_upload_epis_u16(rslf_volume* vol, const uint16_t* const* h_epis, size_t row_stride_bytes,
                                           float epi_scale_factor, float* scale_used) RSLF_API_TRY
{
    return upload_epis_elem(vol, Elem::U16, (const void* const*)h_epis, row_stride_bytes, epi_scale_factor, scale_used);
}
RSLF_API_CATCH

extern "C" int rslf_volume_upload_images_f32(rslf_volume* vol, const float* const* h_imgs, size_t row_stride_bytes,
                                             float epi_scale_factor, float* scale_used) RSLF_API_TRY
{
    return upload_images_elem(vol, Elem::F32, (const void* const*)h_imgs, row_stride_bytes, epi_scale_factor, scale_used);
}
RSLF_API_CATCH

extern "C" int rslf_volume_upload_images_u8(rslf_volume* vol, const uint8_t* const* h_imgs, size_t row_stride_bytes) RSLF_API_TRY
{
    return upload_images_elem(vol, Elem::U8, (const void* const*)h_imgs, row_stride_bytes, -1.0f, nullptr);
}
RSLF_API_CATCH

extern "C" int rslf_volume_upload_images_u16(rslf_volume* vol, const uint16_t* const* h_imgs, size_t row_stride_bytes,
                                             float epi_scale_factor, float* scale_used) RSLF_API_TRY
{
    return upload_images_elem(vol, Elem::U16, (const void* const*)h_imgs, row_stride_bytes, epi_scale_factor, scale_used);
}
RSLF_API_CATCH

extern "C" int rslf_volume_upload_images_xf_f32(rslf_volume* vol, const float* const* h_imgs, size_t row_stride_bytes,
                                                float epi_scale_factor, float* scale_used, int transpose, int rotate_180) RSLF_API_TRY
{
    return upload_images_xf_elem(vol, Elem::F32, (const void* const*)h_imgs, row_stride_bytes, epi_scale_factor, scale_used, transpose,
                                 rotate_180);
}
RSLF_API_CATCH

extern "C" int rslf_volume_upload_images_xf_u8(rslf_volume* vol, const uint8_t* const* h_imgs, size_t row_stride_bytes, int transpose,
                                               int rotate_180) RSLF_API_TRY
{
    return upload_images_xf_elem(vol, Elem::U8, (const void* const*)h_imgs, row_stride_bytes, -1.0f, nullptr, transpose, rotate_180);
}
RSLF_API_CATCH

extern "C" int rslf_volume_upload_images_xf_u16(rslf_volume* vol, const uint16_t* const* h_imgs, size_t row_stride_bytes,
                                                float epi_scale_factor, float* scale_used, int transpose, int rotate_180) RSLF_API_TRY
{
    return upload_images_xf_elem(vol, Elem::U16, (const void* const*)h_imgs, row_stride_bytes, epi_scale_factor, scale_used, transpose,
                                 rotate_180);
}
RSLF_API_CATCH

extern "C" int rslf_volume_pack_device_f32(rslf_volume* vol, const float* d_vsuc, float epi_scale_factor, float* scale_used) RSLF_API_TRY
{
    if (!vol || !d_vsuc)
        return fail(RSLF_ERR_INVALID_ARG, "vol/d_vsuc is NULL");
    if (epi_scale_factor < 0)
        return fail(RSLF_ERR_INVALID_ARG, "pack_device needs an explicit epi_scale_factor (> 0); 1.0 keeps the values");
    rslf_ctx* ctx = vol->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if (scale_used)
        *scale_used = epi_scale_factor;
    int rc = minmax_begin(ctx);
    if (rc)
        return rc;
    rc = pack_chunk<float>(vol, d_vsuc, 0, vol->V, false, scale_of(epi_scale_factor));
    if (rc)
        return rc;
    return minmax_end(vol);
}
RSLF_API_CATCH

template int rslf::upload_host<float>(rslf_volume*, const float* const*, size_t, bool, float);
template int rslf::upload_host<uint8_t>(rslf_volume*, const uint8_t* const*, size_t, bool, float);
template int rslf::upload_host<uint16_t>(rslf_volume*, const uint16_t* const*, size_t, bool, float);

// dc.hpp:442-460 over all EPIs, by up to eight host threads
template <typename T>
float rslf::host_max_parallel(const T* const* h_epis, int V, int S, size_t stride, size_t row_elems, float start)
{
    const int nt = std::max(1, std::min<int>(8, std::min<int>((int)std::thread::hardware_concurrency(), V / 8)));
    std::vector<float> part((size_t)nt, start);
    {
        JoinGuard pool;
        for (int t = 0; t < nt; t++)
            pool.run([&, t] {
                int v0, v1;
                plan::split_range(V, t, nt, &v0, &v1);
                part[(size_t)t] = host_max(h_epis + v0, v1 - v0, S, stride, row_elems, start);
            });
    }
    float m = start;
    for (int t = 0; t < nt; t++)
        m = std::max(m, part[(size_t)t]);
    return m;
}
template float rslf::host_max_parallel<float>(const float* const*, int, int, size_t, size_t, float);
template float rslf::host_max_parallel<uint16_t>(const uint16_t* const*, int, int, size_t, size_t, float);
