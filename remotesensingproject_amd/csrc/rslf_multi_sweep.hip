// librslf_hip.so, unit 9 of 9: the 2-D sweep sharded by scanline over the devices of one process, behind the C-ABI -- one
// neighbour exchange of boundary rows per visit (the path's one real exchange step) -- and fine-to-coarse with every level
// swept so (the level loop itself is rslf_f2c.hip's).  C-ABI: include/rslf_hip.h.
#include "rslf_internal.hpp"

#include <algorithm>
#include <cmath>
#include <optional>
#include <stdexcept>

using namespace rslf;

// ---- Depth2DComputer::run over several devices (dc.hpp:748-805) -----------------------------------------------------
// The 2-D sweep sharded by scanline behind the C-ABI: every device holds a block of scanlines (+ the median's halo) of the
// volume and of the [S][rows][U] planes; a visit is scan on every device, then the neighbours' boundary rows of the visited
// view's raw disparities and edge mask by peer copy (the one real exchange step of the path, as sharding.ShardedDepth2D
// does it over RCCL), then median + propagation on every device.  ONE host thread drives all devices: every call only
// queues work, the order between devices is kept by events -- a device's finish waits for its neighbours to have
// fetched its boundary rows, because the apply pass rewrites them (core.hpp:1119-1121).
namespace {

// One device's part of one sweep.  It owns what it holds: however the sweep ends -- completed, an early return, an exception --
// the destructor ends a sweep still open as failed, waits for the stream, puts the context's stream back and destroys the
// volume and the events.  (The planes live in the device's arena, which stays.)
struct Sweep2DDev {
    rslf_ctx* ctx = nullptr;            // set once the device is taken up; nothing to undo before
    std::optional<StreamScope> on;      // the context works on the device's compute stream while the sweep lasts
    rslf_volume* vol = nullptr;
    float *Ce = nullptr, *Cd = nullptr, *depth = nullptr, *rbar = nullptr;
    float *dmin = nullptr, *dmax = nullptr;   // per-pixel hypothesis ranges over the held rows (a fine-to-coarse level), or NULL
    uint8_t *cem = nullptr, *scan_mask = nullptr;
    int lo = 0, hi = 0, a = 0, b = 0;   // rows held [lo, hi), rows owned [a, b)
    hipEvent_t ev_scan = nullptr, ev_fetch = nullptr;
    bool begun = false;

    Sweep2DDev() = default;
    Sweep2DDev(const Sweep2DDev&) = delete;
    Sweep2DDev& operator=(const Sweep2DDev&) = delete;
    ~Sweep2DDev()
    {
        if (!ctx)
            return;
        (void)hipSetDevice(ctx->device);
        if (begun)
            (void)rslf_sweep_end(ctx, 0, 2, nullptr);
        (void)hipStreamSynchronize(ctx->stream);
        on.reset();
        if (vol)
            (void)rslf_volume_destroy(vol);
        if (ev_scan)
            (void)hipEventDestroy(ev_scan);
        if (ev_fetch)
            (void)hipEventDestroy(ev_fetch);
    }
    plan::RowBlock block() const { return plan::RowBlock{a, b, lo, hi}; }
    // rows of plane `base` ([S][rows][U] elements of `esz` bytes) of view s_hat, from local row r on
    char* rows_of(void* base, size_t esz, int s_hat, int r, int U) const { return (char*)base + (((size_t)s_hat * (hi - lo) + r) * U) * esz; }
};

// The fine-to-coarse form of a sweep: nothing passes through host memory.  The level's RAW volume, its per-pixel ranges
// and the two planes the next steps need live on the FIRST device; every device takes the rows it holds from there and
// leaves its own rows of the results there, by peer copies (plain device copies where it is the first device itself).
struct FirstDevicePlanes {
    const float* raw_vsuc = nullptr;   // [V][S][U][C] raw values of the level (replaces the host EPIs)
    const float* dmin_svu = nullptr;   // [S][V][U] ranges, or NULL for the scalar range
    const float* dmax_svu = nullptr;
    float* Ce_svu = nullptr;           // [S][V][U] results
    float* depth_svu = nullptr;
};

// What every part of one sweep is told: the field, the scan's arguments and where the results go.
struct Sweep2DJob {
    rslf_multi* m;
    const void* const* h_epis;
    Elem elem;
    size_t row_stride_bytes;
    int V, S, U, C;
    float scale_arg, dmin, dmax;
    int dim_d;
    const rslf_params* p;
    const FirstDevicePlanes* first;   // or NULL
    float *h_Ce, *h_Cd, *h_depth, *h_rbar;   // the caller's [S][V][U] planes (a NULL one is not wanted)
    uint8_t *h_Ce_mask, *h_scan_mask;
    int nd, h_med, halo;              // devices that take part, the median's halo, the rows a block holds beyond its own
};

// Device i takes its rows: volume, planes, edge confidence, sweep state.
int sweep2d_setup(const Sweep2DJob& j, int i, Sweep2DDev& d)
{
    rslf_multi::Dev& md = j.m->devs[(size_t)i];
    rslf_ctx* ctx = md.ctx;
    const FirstDevicePlanes* first = j.first;
    const bool ranges = first && first->dmin_svu;
    const int dev0 = j.m->devs[0].ctx->device, S = j.S, U = j.U, C = j.C;
    HIP_TRY(hipSetDevice(ctx->device));
    d.ctx = ctx;
    d.on.emplace(ctx, md.s_comp);
    const plan::RowBlock blk = plan::row_block(j.V, i, j.nd, j.halo);
    d.a = blk.a, d.b = blk.b, d.lo = blk.lo, d.hi = blk.hi;
    const int rows = d.hi - d.lo;
    const size_t n = (size_t)S * rows * U;
    HIP_TRY(hipEventCreateWithFlags(&d.ev_scan, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&d.ev_fetch, hipEventDisableTiming));
    int rc = rslf_volume_create(ctx, rows, S, U, C, &d.vol);
    if (rc)
        return rc;
    // a copy between this device and the first one (either direction), queued on this device's stream
    auto copy01 = [&](void* dst, int dst_dev, const void* src, int src_dev, size_t bytes) -> hipError_t {
        return multi_copy(j.m, dst, dst_dev, src, src_dev, bytes, ctx->stream);
    };
    if (first && first->raw_vsuc) {   // the held rows of the level's raw volume: from the first device
        const size_t row_floats = (size_t)S * U * C;
        const float* src = first->raw_vsuc + (size_t)d.lo * row_floats;
        if (ctx->device != dev0) {
            rc = ensure_staging(ctx, (size_t)rows * row_floats * sizeof(float));
            if (rc)
                return rc;
            HIP_TRY(copy01(ctx->scratch.staging.get(), ctx->device, src, dev0, (size_t)rows * row_floats * sizeof(float)));
            src = ctx->scratch.staging.as<const float>();
        }
        rc = rslf_volume_pack_device_f32(d.vol, src, j.scale_arg, nullptr);
    } else {
        rc = upload_host_elem(d.vol, j.elem, j.h_epis + d.lo, j.row_stride_bytes, false, scale_of(j.scale_arg));
    }
    if (rc)
        return rc;
    {   // planes: one allocation per device, grown when a larger field comes (allocation calls synchronise the device)
        const size_t nf = (n + 63) & ~(size_t)63;   // floats per plane, 256-byte aligned
        const size_t need = nf * sizeof(float) * (3 + (size_t)C + (ranges ? 2 : 0)) + 2 * nf;
        HIP_TRY(hip_err(md.arena.reserve(need)));
        float* f = md.arena.as<float>();
        d.Ce = f, f += nf;
        d.Cd = f, f += nf;
        d.depth = f, f += nf;
        d.rbar = f, f += nf * C;
        if (ranges) {
            d.dmin = f, f += nf;
            d.dmax = f, f += nf;
        }
        d.cem = reinterpret_cast<uint8_t*>(f);
        d.scan_mask = d.cem + nf;
    }
    hipStream_t st = ctx->stream;
    if (ranges) {   // the held rows of every view's range planes: one run of bytes per view
        const size_t w = (size_t)rows * U;
        for (int sv = 0; sv < S; sv++) {
            HIP_TRY(copy01(d.dmin + (size_t)sv * w, ctx->device, first->dmin_svu + ((size_t)sv * j.V + d.lo) * U, dev0, w * sizeof(float)));
            HIP_TRY(copy01(d.dmax + (size_t)sv * w, ctx->device, first->dmax_svu + ((size_t)sv * j.V + d.lo) * U, dev0, w * sizeof(float)));
        }
    }
    HIP_TRY(hipMemsetAsync(d.Ce, 0, n * sizeof(float), st));   // dc.hpp:733-750
    HIP_TRY(hipMemsetAsync(d.Cd, 0, n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(d.depth, 0, n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(d.rbar, 0, n * C * sizeof(float), st));
    rc = rslf_edge_confidence_2d(ctx, d.vol, j.p, d.Ce, d.cem);                               // dc.hpp:772
    if (rc)
        return rc;
    rc = rslf_sweep_begin(ctx, d.vol, d.cem, d.scan_mask, j.dim_d, d.a - d.lo, d.b - d.lo);  // dc.hpp:780
    d.begun = rc == RSLF_OK;
    return rc;
}

// One op of a visit's schedule (plan::sweep_visit_schedule) on its device: the waits for the neighbours' events, then the
// scan, the fetch of one neighbour's boundary rows, or the finish.
int sweep2d_queue(const Sweep2DJob& j, std::vector<Sweep2DDev>& ds, const plan::VisitOp& op, int s_hat)
{
    Sweep2DDev& d = ds[(size_t)op.dev];
    rslf_ctx* ctx = d.ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    for (int k : op.wait_scan_of)
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ds[(size_t)k].ev_scan, 0));
    for (int k : op.wait_fetch_of)
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ds[(size_t)k].ev_fetch, 0));
    if (op.kind == plan::VisitOp::SCAN) {
        int rc = rslf_sweep_visit_scan(ctx, d.vol, d.dmin, d.dmax, j.dmin, j.dmax, j.dim_d, s_hat, d.Ce, d.cem, d.Cd, d.depth, d.rbar, j.p);
        if (rc)
            return rc;
        HIP_TRY(hipEventRecord(d.ev_scan, ctx->stream));
        if (j.h_med == 0 || j.nd == 1)
            HIP_TRY(hipEventRecord(d.ev_fetch, ctx->stream));   // nothing to fetch: the event the neighbours' finish waits for
        return RSLF_OK;
    }
    if (op.kind == plan::VisitOp::FETCH) {
        const Sweep2DDev& o = ds[(size_t)op.neighbour];
        int dst_r, src_r;
        plan::fetch_rows(d.block(), o.block(), op.neighbour < op.dev ? 0 : 1, j.h_med, &dst_r, &src_r);
        for (int pl = 0; pl < 2; pl++) {   // the visited view's raw disparities and its edge mask
            const size_t esz = pl == 0 ? sizeof(float) : 1;
            char* dst = d.rows_of(pl == 0 ? (void*)d.depth : (void*)d.cem, esz, s_hat, dst_r, j.U);
            const char* src = o.rows_of(pl == 0 ? (void*)o.depth : (void*)o.cem, esz, s_hat, src_r, j.U);
            HIP_TRY(multi_copy(j.m, dst, ctx->device, src, o.ctx->device, (size_t)j.h_med * j.U * esz, ctx->stream));
        }
        HIP_TRY(hipEventRecord(d.ev_fetch, ctx->stream));   // re-recorded after each fetch: the LAST one is what counts
        return RSLF_OK;
    }
    return rslf_sweep_visit_finish(ctx, d.vol, s_hat, d.cem, d.Cd, d.depth, d.rbar, j.p);
}

// The device's sweep ends well (its stats to st), and its own rows of every view are queued to their place in the
// caller's [S][V][U] planes.
int sweep2d_collect(const Sweep2DJob& j, Sweep2DDev& d, rslf_stats* st)
{
    rslf_ctx* ctx = d.ctx;
    const int S = j.S, U = j.U, V = j.V, dev0 = j.m->devs[0].ctx->device;
    HIP_TRY(hipSetDevice(ctx->device));
    d.begun = false;
    int rc = rslf_sweep_end(ctx, 1, j.dim_d, st);
    if (rc)
        return rc;
    const int rows = d.hi - d.lo, own = d.b - d.a;
    if (j.first && j.first->Ce_svu) {   // this device's own rows of the two planes the next steps read: to the first device
        const size_t w = (size_t)own * U;
        for (int sv = 0; sv < S; sv++) {
            const size_t src = ((size_t)sv * rows + (d.a - d.lo)) * U, dst = ((size_t)sv * V + d.a) * U;
            HIP_TRY(multi_copy(j.m, j.first->Ce_svu + dst, dev0, d.Ce + src, ctx->device, w * sizeof(float), ctx->stream));
            HIP_TRY(multi_copy(j.m, j.first->depth_svu + dst, dev0, d.depth + src, ctx->device, w * sizeof(float), ctx->stream));
        }
    }
    const struct {   // the six planes: the caller's, the device's, bytes per pixel
        void* host;
        const void* dev;
        size_t esz;
    } planes[6] = {{j.h_Ce, d.Ce, 4},       {j.h_Ce_mask, d.cem, 1},           {j.h_Cd, d.Cd, 4},
                   {j.h_depth, d.depth, 4}, {j.h_rbar, d.rbar, 4 * (size_t)j.C}, {j.h_scan_mask, d.scan_mask, 1}};
    for (const auto& q : planes)
        if (q.host)
            HIP_TRY(hipMemcpy2DAsync((char*)q.host + (size_t)d.a * U * q.esz, (size_t)V * U * q.esz, (const char*)q.dev + (size_t)(d.a - d.lo) * U * q.esz,
                                     (size_t)rows * U * q.esz, (size_t)own * U * q.esz, S, hipMemcpyDeviceToHost, ctx->stream));
    return RSLF_OK;
}

int multi_depth2d(rslf_multi* m, const void* const* h_epis, Elem elem, size_t row_stride_bytes, int V, int S, int U, int C, float scale_arg,
                  float dmin, float dmax, int dim_d, const rslf_params* p, float* h_Ce_svu, uint8_t* h_Ce_mask_svu, float* h_Cd_svu,
                  float* h_depth_svu, float* h_rbar_svu, uint8_t* h_scan_mask_svu, rslf_stats* stats,
                  const FirstDevicePlanes* first = nullptr)
{
    if (!m || (!h_epis && !(first && first->raw_vsuc)))
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (first && ((first->dmin_svu == nullptr) != (first->dmax_svu == nullptr)))
        return fail(RSLF_ERR_INVALID_ARG, "dmin_svu and dmax_svu must both be given or both be NULL");
    if (V < 1 || S < 1 || U < 1 || (C != 1 && C != 3))
        return fail(RSLF_ERR_INVALID_ARG, "bad dimensions V=%d S=%d U=%d C=%d", V, S, U, C);
    int rc = check_params(p);
    if (rc)
        return rc;
    for (int v = 0; h_epis && v < V; v++)
        if (!h_epis[v])
            return fail(RSLF_ERR_INVALID_ARG, "h_epis[%d] is NULL", v);
    const int h_med = plan::median_halo(p->median_filter_size);
    const int halo = plan::halo_rows(p->median_filter_size, p->edge_confidence_opening_size);
    const int nd = plan::sweep_devices_for(V, (int)m->devs.size(), halo);   // a block must be able to fill its neighbours' halo rows
    const Sweep2DJob j = {m, h_epis, elem, row_stride_bytes, V, S, U, C, scale_arg, dmin, dmax, dim_d, p, first,
                          h_Ce_svu, h_Cd_svu, h_depth_svu, h_rbar_svu, h_Ce_mask_svu, h_scan_mask_svu, nd, h_med, halo};
    std::vector<Sweep2DDev> ds((size_t)nd);   // sized once; whatever path leaves this function, the destructors clean up
    for (int i = 0; i < nd; i++) {
        rc = sweep2d_setup(j, i, ds[(size_t)i]);
        if (rc)
            return rc;
    }
    if (inject_hit(kInjectSweep))
        throw std::runtime_error("injected failure in a sharded sweep (rslf_debug_inject)");
    // One visit = plan::sweep_visit_schedule: scan on every device; every device fetches its neighbours' boundary rows
    // (after the neighbour's scan); every device finishes once BOTH neighbours have fetched its raw rows (its apply pass
    // rewrites them, core.hpp:1119-1121).  One host thread queues the ops; the waits are events between streams.
    const std::vector<plan::VisitOp> schedule = plan::sweep_visit_schedule(nd, h_med);
    for (int s_hat : plan::sweep_order(S))   // core.hpp:981-990
        for (const plan::VisitOp& op : schedule) {
            rc = sweep2d_queue(j, ds, op, s_hat);
            if (rc)
                return rc;
        }
    long long scanned = 0;
    for (int i = 0; i < nd; i++) {
        rslf_stats st_i;
        memset(&st_i, 0, sizeof(st_i));
        rc = sweep2d_collect(j, ds[(size_t)i], &st_i);
        if (rc)
            return rc;
        scanned += st_i.pixels_scanned;
        if (stats && i == 0) {
            stats->scan_kernel = st_i.scan_kernel;
            stats->s_pad = st_i.s_pad;
        }
    }
    for (const Sweep2DDev& d : ds) {
        HIP_TRY(hipSetDevice(d.ctx->device));
        HIP_TRY(hipStreamSynchronize(d.ctx->stream));
    }
    if (stats) {
        stats->pixels_scanned = scanned;
        stats->units = scanned * dim_d;
    }
    return RSLF_OK;
}

}  // namespace

// FineToCoarse<T> (rslf_fine_to_coarse.hpp:103-324) over the object's devices: the level loop of rslf_f2c.hip on the first
// device, where each level's raw volume, ranges, disparities and confidences live; each level's 2-D sweep -- where the
// time goes -- runs sharded (multi_depth2d), the devices taking their rows from there and leaving their results there by
// peer copies (FirstDevicePlanes).  The host sees the EPIs going up once and the fused map coming down.
static int multi_fine_to_coarse(rslf_multi* m, const F2cRequest& req, const F2cOptions& options, const F2cHostOut& out, rslf_stats* stats)
{
    if (!m)
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    if (options.derivative_weight != 0.0f)   // before a device is touched
        return fail(RSLF_ERR_INVALID_ARG, "derivative_channels=%g is not built here (the pyramid's derivative channels are built for one device)",
                    (double)options.derivative_weight);
    if (options.equalize_mode != 0)
        return fail(RSLF_ERR_INVALID_ARG, "equalize_views=%d is not built here (a view's statistic spans all scanlines: the pyramid's "
                    "equalisation is built for one device)", options.equalize_mode);
    if (options.level_dilation != 1)
        return fail(RSLF_ERR_INVALID_ARG, "level_dilation=%d is not built here (the pyramid's level dilation is built for one device)",
                    options.level_dilation);
    rslf_ctx* ctx = m->devs[0].ctx;
    auto sweep = [&](const F2cLevel& lv, rslf_stats* level_stats) -> int {
        if (lv.options->peaks)   // (and with them the validity by uniqueness, which reads them)
            return fail(RSLF_ERR_INVALID_ARG, "peaks: the pyramid's peak planes and its uniqueness ratio are built for one device");
        if (lv.options->cs_min_agree)
            return fail(RSLF_ERR_INVALID_ARG, "consistency_min_agree: the pyramid's validity by cross-view consistency is built for one device");
        const FirstDevicePlanes first{lv.raw_vsuc, lv.dmin_svu, lv.dmax_svu, lv.Ce_svu, lv.depth_svu};
        HIP_TRY(hipStreamSynchronize(ctx->stream));   // what the other devices' streams are about to read is complete
        int rc = multi_depth2d(m, nullptr, Elem::F32, 0, lv.V, req.S, lv.U, req.C, lv.scale, req.d_min, req.d_max, req.dim_d, &lv.params,
                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, level_stats, &first);
        if (rc)
            return rc;
        HIP_TRY(hipSetDevice(ctx->device));
        return RSLF_OK;
    };
    return fine_to_coarse(ctx, req, options, out, stats, nullptr, sweep);
}

extern "C" int rslf_multi_fine_to_coarse_run_host(rslf_multi* m, const void* const* h_epis, int is_u8, int V, int S, int U, int C,
                                                  size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                                  const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                                  float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels, rslf_stats* stats) RSLF_API_TRY
{
    const F2cRequest req = {is_u8 ? Elem::U8 : Elem::F32, h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p,
                            max_pyr_depth, accept_all_last_scale};
    return multi_fine_to_coarse(m, req, F2cOptions(), {h_out_map_svu, h_out_valid_svu, n_levels, nullptr}, stats);
}
RSLF_API_CATCH

extern "C" int rslf_multi_fine_to_coarse_run_host_u16(rslf_multi* m, const uint16_t* const* h_epis, int V, int S, int U, int C,
                                                      size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                                      const rslf_params* p, int max_pyr_depth, int accept_all_last_scale,
                                                      float* h_out_map_svu, uint8_t* h_out_valid_svu, int* n_levels,
                                                      rslf_stats* stats) RSLF_API_TRY
{
    const F2cRequest req = {Elem::U16, (const void* const*)h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p,
                            max_pyr_depth, accept_all_last_scale};
    return multi_fine_to_coarse(m, req, F2cOptions(), {h_out_map_svu, h_out_valid_svu, n_levels, nullptr}, stats);
}
RSLF_API_CATCH

// Depth2DComputer from host EPIs of element type e; the default scale is the maximum over ALL EPIs, taken once
// (dc.hpp:671-705, resolve_scale_factor).
static int multi_depth2d_host(rslf_multi* m, Elem e, const void* const* h_epis, size_t row_stride_bytes, int V, int S, int U, int C,
                              float epi_scale_factor, float dmin, float dmax, int dim_d, const rslf_params* p, float* h_Ce_svu,
                              uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu, float* h_rbar_svu, uint8_t* h_scan_mask_svu,
                              rslf_stats* stats, float* scale_used)
{
    if (!m || !h_epis || V < 1 || S < 1 || U < 1 || (C != 1 && C != 3))
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument or bad dimensions V=%d S=%d U=%d C=%d", V, S, U, C);
    const size_t row_elems = (size_t)U * C;
    const size_t row_bytes = row_elems * elem_bytes(e);
    const size_t stride = row_stride_bytes ? row_stride_bytes : row_bytes;
    if (stride < row_bytes)
        return fail(RSLF_ERR_INVALID_ARG, "row_stride_bytes %zu < row size %zu", stride, row_bytes);
    for (int v = 0; v < V; v++)
        if (!h_epis[v])
            return fail(RSLF_ERR_INVALID_ARG, "h_epis[%d] is NULL", v);
    epi_scale_factor = resolve_scale_factor(e, h_epis, V, S, stride, row_elems, epi_scale_factor, true);
    if (scale_used)
        *scale_used = epi_scale_factor;
    return multi_depth2d(m, h_epis, e, stride, V, S, U, C, epi_scale_factor, dmin, dmax, dim_d, p, h_Ce_svu, h_Ce_mask_svu, h_Cd_svu,
                         h_depth_svu, h_rbar_svu, h_scan_mask_svu, stats);
}

extern "C" int rslf_multi_depth2d_run_f32(rslf_multi* m, const float* const* h_epis, size_t row_stride_bytes, int V, int S, int U, int C,
                                          float epi_scale_factor, float dmin, float dmax, int dim_d, const rslf_params* p,
                                          float* h_Ce_svu, uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu,
                                          float* h_rbar_svu, uint8_t* h_scan_mask_svu, rslf_stats* stats, float* scale_used) RSLF_API_TRY
{
    return multi_depth2d_host(m, Elem::F32, (const void* const*)h_epis, row_stride_bytes, V, S, U, C, epi_scale_factor, dmin, dmax, dim_d,
                              p, h_Ce_svu, h_Ce_mask_svu, h_Cd_svu, h_depth_svu, h_rbar_svu, h_scan_mask_svu, stats, scale_used);
}
RSLF_API_CATCH

extern "C" int rslf_multi_depth2d_run_u8(rslf_multi* m, const uint8_t* const* h_epis, size_t row_stride_bytes, int V, int S, int U, int C,
                                         float dmin, float dmax, int dim_d, const rslf_params* p, float* h_Ce_svu,
                                         uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu, float* h_rbar_svu,
                                         uint8_t* h_scan_mask_svu, rslf_stats* stats) RSLF_API_TRY
{
    // (the argument checks, the stride's among them, are multi_depth2d_host's; its scale for CV_8U is 255)
    return multi_depth2d_host(m, Elem::U8, (const void* const*)h_epis, row_stride_bytes, V, S, U, C, -1.0f, dmin, dmax, dim_d, p,
                              h_Ce_svu, h_Ce_mask_svu, h_Cd_svu, h_depth_svu, h_rbar_svu, h_scan_mask_svu, stats, nullptr);
}
RSLF_API_CATCH

extern "C" int rslf_multi_depth2d_run_u16(rslf_multi* m, const uint16_t* const* h_epis, size_t row_stride_bytes, int V, int S, int U, int C,
                                          float epi_scale_factor, float dmin, float dmax, int dim_d, const rslf_params* p,
                                          float* h_Ce_svu, uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu,
                                          float* h_rbar_svu, uint8_t* h_scan_mask_svu, rslf_stats* stats, float* scale_used) RSLF_API_TRY
{
    return multi_depth2d_host(m, Elem::U16, (const void* const*)h_epis, row_stride_bytes, V, S, U, C, epi_scale_factor, dmin, dmax, dim_d,
                              p, h_Ce_svu, h_Ce_mask_svu, h_Cd_svu, h_depth_svu, h_rbar_svu, h_scan_mask_svu, stats, scale_used);
}
RSLF_API_CATCH
