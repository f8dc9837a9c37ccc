// librslf_hip.so, unit 2 of 9: the hot path -- edge confidence (K1), the scan (K2), the selective median (K3) and the
// Depth1DComputer / Depth1DComputer_pile drivers over them.  C-ABI: include/rslf_hip.h.
#include "rslf_internal.hpp"

#include <algorithm>
#include <cmath>

#include "k1_edge.hpp"
#include "k2_scan.hpp"
#include "k2_reg.hpp"
#include "k2_stream.hpp"
#include "k3_median.hpp"

using namespace rslf;

static_assert(sizeof(Partial) == plan::kPartialRecordBytes, "rslf_plan.hpp sizes the record scratch");
static_assert(kScanWaves == plan::kScanWavesPerTile, "rslf_plan.hpp shares the hypotheses out over this many waves");
static_assert(!RSLF_SCALAR_TAPS || !RSLF_TAP_TABLE || (scan_reg_scalar_taps(104, 1) && row_exact_slots(104, 1) == 104),
              "rslf_internal.hpp names the kernel that has the scalar-tap form");

// ---- hot path -------------------------------------------------------------

extern "C" int rslf_edge_confidence_pile(rslf_ctx* ctx, const rslf_volume* vol, int s, const rslf_params* p,
                                         float* d_Ce_vu, uint8_t* d_Ce_mask_vu) RSLF_API_TRY
{
    if (!ctx || !vol || !d_Ce_vu || !d_Ce_mask_vu)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    int rc = check_params(p);
    if (rc)
        return rc;
    if (s < 0 || s >= vol->S)
        return fail(RSLF_ERR_INVALID_ARG, "s=%d outside [0,%d)", s, vol->S);
    if (!vol->filled)
        return fail(RSLF_ERR_INVALID_ARG, "volume has not been filled");
    HIP_TRY(hipSetDevice(ctx->device));
    EdgeConsts ec;
    ec.filter_size = p->edge_confidence_filter_size;
    ec.cut_shadows = p->cut_shadows;
    ec.shadow_level = p->shadow_level;
    ec.edge_thr = p->edge_score_threshold;
    const dim3 grid((vol->U + 255) / 256, vol->V);
    if (vol->C == 1)
        hipLaunchKernelGGL(k1_edge_confidence<1>, grid, dim3(256), 0, ctx->stream, view_of(vol), s, ec, d_Ce_vu, d_Ce_mask_vu);
    else
        hipLaunchKernelGGL(k1_edge_confidence<3>, grid, dim3(256), 0, ctx->stream, view_of(vol), s, ec, d_Ce_vu, d_Ce_mask_vu);
    HIP_TRY(hipGetLastError());
    if (p->edge_confidence_opening_size > 1) {   // core.hpp:759-768
        rc = ensure_plane_scratch(ctx, vol->V, vol->U);
        if (rc)
            return rc;
        const MorphElement el = plan::structuring_element(p->edge_confidence_opening_type, p->edge_confidence_opening_size);
        uint8_t* tmp = ctx->scratch.morph_tmp();
        hipLaunchKernelGGL(k1_morph_pass, grid, dim3(256), 0, ctx->stream, d_Ce_mask_vu, tmp, vol->V, vol->U, el, 0);   // erode
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k1_morph_pass, grid, dim3(256), 0, ctx->stream, tmp, d_Ce_mask_vu, vol->V, vol->U, el, 1);   // dilate
        HIP_TRY(hipGetLastError());
    }
    return RSLF_OK;
}
RSLF_API_CATCH

// Edge confidence of every view in one launch (the 2-D sweep's first step, core.hpp:918-934)
extern "C" int rslf_edge_confidence_2d(rslf_ctx* ctx, const rslf_volume* vol, const rslf_params* p, float* d_Ce_svu,
                                       uint8_t* d_Ce_mask_svu) RSLF_API_TRY
{
    if (!ctx || !vol || !d_Ce_svu || !d_Ce_mask_svu)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    const size_t n = (size_t)vol->V * vol->U;
    if (p && p->edge_confidence_opening_size <= 1 && vol->S <= 65535 && vol->V <= 65535) {   // every view in one launch
        int rc = check_params(p);
        if (rc)
            return rc;
        if (!vol->filled)
            return fail(RSLF_ERR_INVALID_ARG, "volume has not been filled");
        HIP_TRY(hipSetDevice(ctx->device));
        EdgeConsts ec;
        ec.filter_size = p->edge_confidence_filter_size;
        ec.cut_shadows = p->cut_shadows;
        ec.shadow_level = p->shadow_level;
        ec.edge_thr = p->edge_score_threshold;
        const dim3 grid((vol->U + 255) / 256, vol->V, vol->S);
        if (vol->C == 1)
            hipLaunchKernelGGL(k1_edge_confidence_views<1>, grid, dim3(256), 0, ctx->stream, view_of(vol), ec, d_Ce_svu, d_Ce_mask_svu);
        else
            hipLaunchKernelGGL(k1_edge_confidence_views<3>, grid, dim3(256), 0, ctx->stream, view_of(vol), ec, d_Ce_svu, d_Ce_mask_svu);
        HIP_TRY(hipGetLastError());
        return RSLF_OK;
    }
    for (int s = 0; s < vol->S; s++) {   // core.hpp:918-934
        int rc = rslf_edge_confidence_pile(ctx, vol, s, p, d_Ce_svu + (size_t)s * n, d_Ce_mask_svu + (size_t)s * n);
        if (rc)
            return rc;
    }
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_selective_median(rslf_ctx* ctx, const rslf_volume* vol, const float* d_src_vu, float* d_dst_vu,
                                     int s_hat, int size, const uint8_t* d_mask_vu, float epsilon) RSLF_API_TRY
{
    if (!ctx || !vol || !d_src_vu || !d_dst_vu || !d_mask_vu)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (d_src_vu == d_dst_vu)
        return fail(RSLF_ERR_INVALID_ARG, "selective median cannot run in place");
    if (size < 0 || size > plan::kMedianMaxSize)
        return fail(RSLF_ERR_INVALID_ARG, "median size %d: must be in [0, %d] (width = (size - 1) / 2, core.hpp:686)", size, plan::kMedianMaxSize);
    if (s_hat < 0 || s_hat >= vol->S)
        return fail(RSLF_ERR_INVALID_ARG, "s_hat=%d outside [0,%d)", s_hat, vol->S);
    HIP_TRY(hipSetDevice(ctx->device));
    const plan::MedianPlan mp = plan::median_plan(size, vol->C);
    const plan::NormThreshold thr = plan::norm_threshold(epsilon);
    const dim3 grid((vol->U + kMedianBlock - 1) / kMedianBlock, vol->V);
    bool launched = false;
#define RSLF_K3_CASE(CC, MODE)                                                                                                   \
    if (!launched && vol->C == CC && mp.mode == MODE) {                                                                           \
        if (mp.lds_bytes > ((size_t)64 << 10))                                                                                    \
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k3_selective_median<CC, MODE>),                           \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)mp.lds_bytes));                         \
        hipLaunchKernelGGL((k3_selective_median<CC, MODE>), grid, dim3(kMedianBlock), mp.lds_bytes, ctx->stream, view_of(vol), d_src_vu, \
                           d_dst_vu, d_mask_vu, s_hat, mp.w, thr);                                                                \
        launched = true;                                                                                                          \
    }
    RSLF_MEDIAN_MODES(RSLF_K3_CASE, 1)
    RSLF_MEDIAN_MODES(RSLF_K3_CASE, 3)
#undef RSLF_K3_CASE
    if (!launched)
        return fail(RSLF_ERR_INTERNAL, "no selective-median kernel for %d channels, mode %d", vol->C, mp.mode);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}
RSLF_API_CATCH

// (the slot counts compiled in: RSLF_SPAD_LIST_* in rslf_plan.hpp)
static int launch_scan_reg(int spad, int C, const ScanArgs& a, dim3 grid, hipStream_t stream)
{
#define RSLF_CASE(N)                                                                                        \
    case N:                                                                                                 \
        if (a.packed && a.px_waves)                                                                         \
            hipLaunchKernelGGL((k2_scan_reg_px<N, RSLF_C>), grid, dim3(64 * kScanWaves), 0, stream, a);     \
        else if (a.packed)                                                                                  \
            hipLaunchKernelGGL((k2_scan_reg_packed<N, RSLF_C>), grid, dim3(64 * kScanWaves), 0, stream, a); \
        else                                                                                                \
            hipLaunchKernelGGL((k2_scan_reg<N, RSLF_C>), grid, dim3(64 * kScanWaves), 0, stream, a);        \
        return RSLF_OK;
    if (C == 1) {
        switch (spad) {
#define RSLF_C 1
            RSLF_SPAD_LIST_1CH(RSLF_CASE)
#undef RSLF_C
        default:
            break;
        }
    } else if (C == 3) {
        switch (spad) {
#define RSLF_C 3
            RSLF_SPAD_LIST_3CH(RSLF_CASE)
#undef RSLF_C
        default:
            break;
        }
    }
#undef RSLF_CASE
    return fail(RSLF_ERR_UNSUPPORTED, "no register scan kernel with %d slots x %d channels", spad, C);
}

// The device headers' numbers for a volume of S views x C channels
static plan::ScanKernelFacts kernel_facts(int S, int C)
{
    const int spad = plan::pick_spad(S, C);
    return plan::ScanKernelFacts{spad ? scan_reg_waves(spad, C) : 0, stream_resident_for(S, C), stream_px_resident_for(S, C)};
}

// The request a scan of V x U pixels makes: the caller's inputs, the context's hooks, and the kernel plan::choose_scan_kernel
// picks (`pixel_ranges`: per-pixel [dmin, dmax] planes, so no one hypothesis grid for all pixels)
static plan::ScanRequest scan_request(const rslf_ctx* ctx, int V, int U, int S, int C, int dim_d, bool in_range, bool linear,
                                      bool pixel_ranges, const ScanInputs& in)
{
    plan::ScanRequest rq = {};
    rq.V = V, rq.U = U, rq.S = S, rq.C = C, rq.dim_d = dim_d;
    rq.num_cus = ctx->num_cus;
    rq.ctx_groups = in.groups;
    rq.ctx_packed = in.packed;
    rq.precompacted = in.lists;
    rq.force_groups = ctx->force_groups;
    rq.force_packed = ctx->force_packed;
    rq.px_mode = ctx->px_mode;
    rq.stream_groups = ctx->stream_groups;
    rq.stream_share = ctx->stream_share;
    rq.stream_lds_bytes = ctx->stream_lds_bytes;
    rq.tap_table = ctx->tap_table;
    const bool dense_uniform = !pixel_ranges && !in.packed && ctx->force_packed != 1 && in.lists != ScanInputs::kPackedList;
    plan::choose_scan_kernel(&rq, in_range, linear, ctx->force_scan, dense_uniform, kernel_facts(S, C));
    rq.scalar_taps = (ctx->scalar_taps && !pixel_ranges && row_exact_slots(rq.spad, C)) ? 1 : 0;   // the kernel has the scalar-tap form
    return rq;
}

// Size the scan's scratch once for pile steps over each of the given scanline counts of an S x U x C volume (the chunks
// of the pipelined host path), assuming radiances in range -- an out-of-range volume runs the generic kernel, whose
// launches take no records.
int rslf::scan_presize(rslf_ctx* ctx, int S, int U, int C, int dim_d, const rslf_params* p, const int* rows, int n_rows)
{
    const plan::ScanKernelFacts f = kernel_facts(S, C);
    int max_rows = 0;
    size_t recs = 0, tickets = 0;
    for (int i = 0; i < n_rows; i++) {
        max_rows = std::max(max_rows, rows[i]);
        ScanInputs in;   // what rslf_depth1d_pile_run passes
        if (p && plan::fuse_k1_compaction(p->edge_confidence_opening_size, ctx->force_packed, (size_t)rows[i] * U))
            in.lists = ScanInputs::kRowLists;
        const plan::ScanRequest rq = scan_request(ctx, rows[i], U, S, C, dim_d, true, !p || p->interpolation == RSLF_INTERP_LINEAR, false, in);
        const plan::ScanPlan sp = plan::plan_scan(rq, f.nres, f.nres_px);
        recs = std::max(recs, sp.records);
        tickets = std::max(tickets, sp.tickets);
    }
    if (max_rows < 1)
        return RSLF_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    bool tickets_fresh = false;
    int rc = ensure_plane_scratch(ctx, max_rows, U);
    if (rc == RSLF_OK && recs)
        rc = ensure_group_scratch(ctx, recs, tickets, &tickets_fresh);
    // fresh tickets are zeroed on the context's CURRENT stream; the caller's launches may go to another one
    if (rc == RSLF_OK && tickets_fresh)
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    return rc;
}

// Size the records of a sweep's sparse visits (`sparse`: what they pass) before its first visit, for linear interpolation
int rslf::sweep_scan_presize(rslf_ctx* ctx, const rslf_volume* vol, int dim_d, const ScanInputs& sparse)
{
    const plan::ScanRequest rq = scan_request(ctx, vol->V, vol->U, vol->S, vol->C, dim_d, plan::scan_range_ok(vol->min_value, vol->max_value),
                                              true, false, sparse);
    size_t recs = 0, tickets = 0;
    plan::sweep_reserve(rq, kernel_facts(vol->S, vol->C), ctx->row_split, &recs, &tickets);
    return recs ? ensure_group_scratch(ctx, recs, tickets) : RSLF_OK;
}

void rslf::fill_stats(rslf_ctx* ctx, unsigned long long tot, int dim_d, rslf_stats* stats)
{
    stats->pixels_scanned = (int64_t)tot;
    stats->units = (int64_t)tot * dim_d;
    stats->scan_kernel = ctx->last_kernel;
    stats->s_pad = ctx->last_spad;
}

// The stats of what the context's stream has been given so far: waits for it and reads the pixel total
int rslf::read_stats(rslf_ctx* ctx, int dim_d, rslf_stats* stats)
{
    unsigned long long tot = 0;
    HIP_TRY(hipMemcpyAsync(&tot, ctx->scratch.pixel_total(), sizeof(tot), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    fill_stats(ctx, tot, dim_d, stats);
    return RSLF_OK;
}

ScanInputs rslf::scan_defaults(const rslf_ctx* ctx)
{
    ScanInputs in;
    in.zero_total = !ctx->sweep.keep_total;             // an open sweep sums its visits' pixels ...
    in.timed = !ctx->sweep.open || ctx->sweep.first;    // ... and times its first visit only
    return in;
}

// The arguments every scan of the hypothesis grid takes (K2, the K columns, the sub-grid refinement)
int rslf::check_scan_args(const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu, int dim_d, int s_hat,
                          const rslf_params* p)
{
    int rc = check_params(p);
    if (rc)
        return rc;
    if ((d_dmin_vu == nullptr) != (d_dmax_vu == nullptr))
        return fail(RSLF_ERR_INVALID_ARG, "d_dmin_vu and d_dmax_vu must both be given or both be NULL");
    if (dim_d < 2)
        return fail(RSLF_ERR_INVALID_ARG, "dim_d=%d: the hypothesis grid divides by dim_d-1 (core.hpp:548)", dim_d);
    if (s_hat < 0 || s_hat >= vol->S)
        return fail(RSLF_ERR_INVALID_ARG, "s_hat=%d outside [0,%d)", s_hat, vol->S);
    if (!vol->filled)
        return fail(RSLF_ERR_INVALID_ARG, "volume has not been filled");
    return RSLF_OK;
}

// The row-exact table of one hypothesis grid and row geometry (k2_taps.hpp, row_exact_entry; read by scan_reg_body_scalar):
// workgroup d fills hypothesis d -- thread s the entry of view s, padding slots the last view's with zero weights -- its disparity, the same
// hypothesis() call as the scan's, and whether every view offset s < S is row-exact.
__global__ __launch_bounds__(128) void k2_fill_row_exact(float dmin, float dmax, int dim_d, float slope, int s_hat, int S, int slots, int U,
                                                         int C, int stride_s, long long* __restrict__ out_off, f2* __restrict__ out_w,
                                                         float* __restrict__ out_D, int* __restrict__ out_exact)
{
    const int d = blockIdx.x, s = threadIdx.x;
    const float Dd = hypothesis(dmin, dmax - dmin, (float)(dim_d - 1), d);
    bool ok = true;
    if (s < slots) {
        // (a padding slot: view S - 1's offset, so that a consumer that loads it reads a valid address, and zero weights)
        const int sv = min(s, S - 1);
        float off = (float)(s_hat - sv) * Dd;   // float(s_hat - s) * D[d]   core.hpp:542,550
        off = off * slope;                      // core.hpp:551
        const RowExactEntry e = row_exact_entry(off, U, C, sv * stride_s);
        const long long bo = (long long)e.byteoff;
        const f2 w = s < S ? f2{e.t, e.omt} : f2{0.0f, 0.0f};
        ok = e.exact;
        out_off[(size_t)d * slots + s] = bo;
        out_w[(size_t)d * slots + s] = w;
    }
    const int all = __syncthreads_and(ok ? 1 : 0);
    if (s == 0) {
        out_D[d] = Dd;
        out_exact[d] = all ? 1 : 0;
    }
}

// Hand the launch its row-exact table where the plan asks for one (one hypothesis grid for all pixels): found in place when
// the context's last table was made from the same key, else filled on the scan's stream, ahead of the scan -- no host-side
// fill, no copy.  The kernels of the stream that still read the old table run before the fill.
static int attach_row_exact(rslf_ctx* ctx, ScanArgs& a, const plan::ScanPlan& p, hipStream_t st)
{
    // (the row kernel itself, and only where it is built with the form: an A/B build without it launches nothing extra)
    const bool has_form = p.kind == RSLF_SCAN_REG && !p.packed && a.vol.C == 1 && p.spad == 104 && scan_reg_scalar_taps(104, 1);
    const int slots = has_form && p.scalar_taps && !a.dmin_vu ? row_exact_slots(p.spad, a.vol.C) : 0;
    ctx->last_row_exact = false;
    if (!slots || a.vol.S > slots || a.vol.S <= slots - 16 || slots > 128 || a.vol.stride_s * (long long)slots > INT32_MAX)
        return RSLF_OK;
    RowExactKey key;
    key.dmin = a.dmin, key.dmax = a.dmax, key.slope = a.k.slope;
    key.dim_d = a.dim_d, key.s_hat = a.s_hat, key.S = a.vol.S, key.U = a.vol.U, key.C = a.vol.C, key.slots = slots;
    key.stride_s = a.vol.stride_s;
    key.queued_on = st;
    const Reserved r = ctx->scratch.row_exact.reserve(row_exact_bytes(a.dim_d, slots));
    if (r.err) {
        ctx->row_exact_key = RowExactKey{};
        HIP_TRY(hip_err(r));
    }
    char* base = ctx->scratch.row_exact.as<char>();
    long long* d_off = reinterpret_cast<long long*>(base);
    f2* d_w = reinterpret_cast<f2*>(d_off + (size_t)a.dim_d * slots);
    float* d_D = reinterpret_cast<float*>(d_w + (size_t)a.dim_d * slots);
    int* d_exact = reinterpret_cast<int*>(d_D + a.dim_d);
    if (r.fresh || !key.same(ctx->row_exact_key)) {
        ctx->row_exact_key = RowExactKey{};
        hipLaunchKernelGGL(k2_fill_row_exact, dim3(a.dim_d), dim3(128), 0, st, a.dmin, a.dmax, a.dim_d, a.k.slope, a.s_hat, a.vol.S, slots,
                           a.vol.U, a.vol.C, (int)a.vol.stride_s, d_off, d_w, d_D, d_exact);
        HIP_TRY(hipGetLastError());
        ctx->row_exact_key = key;
    }
    a.rx_off = d_off;
    a.rx_w = reinterpret_cast<const float*>(d_w);
    a.rx_D = d_D;
    a.rx_exact = d_exact;
    ctx->last_row_exact = true;
    return RSLF_OK;
}

// The launch shape's part of the scan's arguments
static void apply_plan(ScanArgs& a, const plan::ScanPlan& p, const rslf_ctx* ctx)
{
    a.groups = p.groups;
    a.tile_w = p.tile_w;   // the streaming kernel's row tiles leave lane 63 to its neighbour's right tap (DENSE)
    a.tiles_per_row = p.tiles_per_row;
    a.packed = p.packed ? 1 : 0;
    a.packed_adapt = p.packed_adapt ? 1 : 0;
    a.px_waves = p.px_waves;
    a.tap_table = p.tap_table;
    a.stream_park = p.stream_park;
    a.stream_wave_floats = p.stream_wave_floats;
    // grouped launches leave one 32-byte record per (tile, group, lane) for the tile's last group to merge (k2_scan.hpp)
    a.partial = p.groups > 1 ? ctx->scratch.scan_partial.as<Partial>() : nullptr;
    a.ticket = p.groups > 1 ? ctx->scratch.scan_ticket.as<int>() : nullptr;
}

// One launch of the kernel the plan names: its template instantiation for the slot count / resident prefix / channels
// (RSLF_SPAD_LIST_* in rslf_plan.hpp; k2_stream.hpp; the on-chip rungs in rslf_chip_a.hip)
static int enqueue_scan(const plan::ScanPlan& p, const ScanArgs& a, unsigned grid_x, size_t stream_lds_bytes, hipStream_t st)
{
    const dim3 grid(grid_x), block(64 * kScanWaves);
    const int C = a.vol.C;
    hipError_t attr = hipSuccess;
    auto stream = [&](auto kernel) {   // (more than the 64 KiB a kernel gets without asking: set on every launch)
        attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)stream_lds_bytes);
        if (attr == hipSuccess)
            hipLaunchKernelGGL(kernel, grid, block, p.lds_bytes, st, a);
    };
    int rc = RSLF_OK;
    switch (p.kind) {
    case RSLF_SCAN_REG:
    case RSLF_SCAN_REG_PX:
        rc = launch_scan_reg(p.spad, C, a, grid, st);
        break;
    case RSLF_SCAN_CHIP:
        rc = launch_scan_chip(a, grid, p.lds_bytes, st);   // rslf_chip_a.hip: the rung that holds this view count
        break;
    case RSLF_SCAN_STREAM_PX:
        if (C == 1)
            stream_px_kernel_for<1>(p.stream_nres, stream);
        else
            stream_px_kernel_for<3>(p.stream_nres, stream);
        break;
    case RSLF_SCAN_STREAM:
        if (p.packed && C == 1)
            stream_kernel_for<1, true>(p.stream_nres, stream);
        else if (p.packed)
            stream_kernel_for<3, true>(p.stream_nres, stream);
        else if (C == 1)
            stream_kernel_for<1, false>(p.stream_nres, stream);
        else
            stream_kernel_for<3, false>(p.stream_nres, stream);
        break;
    default:
        if (C == 1)
            hipLaunchKernelGGL(k2_scan_generic<1>, grid, block, 0, st, a);
        else
            hipLaunchKernelGGL(k2_scan_generic<3>, grid, block, 0, st, a);
    }
    if (rc)
        return rc;
    HIP_TRY(attr);
    HIP_TRY(hipGetLastError());   // grouped launches merge their records themselves (scan_epilogue): no combine launch
    return RSLF_OK;
}

int rslf::depth_epi_scan(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu, float dmin,
                         float dmax, int dim_d, int s_hat, float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu, float* d_depth_vu,
                         float* d_rbar_vu, const rslf_params* p, uint8_t* d_mask_vu, int32_t* d_idx_vu, float* d_score_vu,
                         rslf_stats* stats, const ScanInputs& in)
{
    if (!ctx || !vol || !d_Ce_vu || !d_Ce_mask_vu || !d_Cd_vu || !d_depth_vu || !d_rbar_vu)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    int rc = check_scan_args(vol, d_dmin_vu, d_dmax_vu, dim_d, s_hat, p);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    rc = ensure_plane_scratch(ctx, vol->V, vol->U);
    if (rc)
        return rc;

    // Kernel and launch shape (rslf_plan.hpp): which kernel, hypothesis groups per tile, packed or row tiles, 63- or 64-entry
    // tiles, row blocks and records of grouped launches, the streaming kernel's LDS split, the grids -- pure host logic,
    // unit-tested on the CPU.  Everything that can fail on the host fails here, before anything is queued.
    const plan::ScanRequest rq = scan_request(ctx, vol->V, vol->U, vol->S, vol->C, dim_d, plan::scan_range_ok(vol->min_value, vol->max_value),
                                              p->interpolation == RSLF_INTERP_LINEAR, d_dmin_vu != nullptr, in);
    const plan::ScanKernelFacts f = kernel_facts(vol->S, vol->C);
    const plan::ScanPlan sp = plan::plan_scan(rq, f.nres, f.nres_px);
    const int row_min = plan::row_split_min(rq, sp, ctx->row_split);
    const plan::ScanPlan spr = row_min ? plan::plan_scan(plan::row_split_request(rq), f.nres) : sp;
    std::vector<plan::ScanLaunch> row_launches, launches;
    long long tiles = 0;
    if (row_min && !plan::scan_launches(vol->V, vol->U, spr, &row_launches, &tiles))
        return fail(RSLF_ERR_UNSUPPORTED, "%lld tiles x %d groups exceeds the grid limit", tiles, spr.groups);
    if (!plan::scan_launches(vol->V, vol->U, sp, &launches, &tiles))
        return fail(RSLF_ERR_UNSUPPORTED, "%lld tiles x %d groups exceeds the grid limit", tiles, sp.groups);
    rc = ensure_group_scratch(ctx, std::max(sp.records, spr.records), std::max(sp.tickets, spr.tickets));
    if (rc)
        return rc;

    const size_t n = (size_t)vol->V * vol->U;
    hipStream_t st = ctx->stream;
    const Scratch& sc = ctx->scratch;
    if (d_idx_vu)
        HIP_TRY(hipMemsetAsync(d_idx_vu, 0xFF, n * sizeof(int32_t), st));   // -1
    if (d_score_vu && in.clear_score)
        HIP_TRY(hipMemsetAsync(d_score_vu, 0, n * sizeof(float), st));
    if (in.zero_total && in.lists == ScanInputs::kCompact)
        HIP_TRY(hipMemsetAsync(sc.pixel_total(), 0, sizeof(unsigned long long), st));
    int* packed_n = sc.packed_len();
    if (in.lists != ScanInputs::kCompact) {
        // nothing to compact
    } else if (sp.packed) {
        if (!in.packed_n_zero)
            HIP_TRY(hipMemsetAsync(packed_n, 0, sizeof(int), st));
        hipLaunchKernelGGL(k_compact_mask_packed, dim3(vol->V), dim3(256), 0, st, d_Ce_mask_vu, d_mask_vu, vol->U, sc.list.as<int>(),
                           sc.count.as<int>(), sc.pixel_total(), packed_n, sc.rowbase.as<int>());
    } else {
        hipLaunchKernelGGL(k_compact_mask, dim3(vol->V), dim3(256), 0, st, d_Ce_mask_vu, d_mask_vu, vol->U, sc.list.as<int>(),
                           sc.count.as<int>(), sc.pixel_total());
    }
    HIP_TRY(hipGetLastError());

    ScanArgs a = {};
    a.vol = view_of(vol);
    a.list = sc.list.as<int>();
    a.count = sc.count.as<int>();
    a.dmin_vu = d_dmin_vu;
    a.dmax_vu = d_dmax_vu;
    a.dmin = dmin;
    a.dmax = dmax;
    a.dim_d = dim_d;
    a.s_hat = s_hat;
    a.k = make_scan_consts(p);
    a.Ce = d_Ce_vu;
    a.Ce_mask = d_Ce_mask_vu;
    a.Cd = d_Cd_vu;
    a.depth = d_depth_vu;
    a.rbar = d_rbar_vu;
    a.idx = d_idx_vu;
    a.score = d_score_vu;
    a.stream_frac_max = plan::stream_frac_max(vol->U);
    a.packed_n = packed_n;
    a.row_min = row_min;
    ScanArgs ar = a;   // the row split's row tiles of the packed list
    apply_plan(a, sp, ctx);
    apply_plan(ar, spr, ctx);
    ar.rowbase = sc.rowbase.as<int>();
    rc = attach_row_exact(ctx, a, sp, st);   // (the row split's tiles belong to stream-class volumes: no register kernel, no table)
    if (rc)
        return rc;
    ctx->last_spad = sp.spad;
    ctx->last_kernel = sp.kind;
    HIP_TRY(hipGetLastError());   // anything an earlier enqueue left behind is not this launch's fault

    // The events that time K2 are marker packets of their own: ~5.6 us each before the next kernel starts (measured,
    // tools/probe_gaps.py) -- nothing beside a 66 ms scan, a tenth of a sweep's sparse visit.  time_all: every launch
    // sequence gets a pair of its own from the pool (rslf_scan_time_total_ms; 32 768 untimed-for launches are the pool's
    // end: later ones go untimed), handed back if the sequence fails to queue.
    const bool pooled = ctx->time_all && ctx->ev_used + 2 <= ((size_t)1 << 16);
    while (pooled && ctx->ev_pool.size() < ctx->ev_used + 2) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreate(&e));
        ctx->ev_pool.push_back(e);
    }
    auto enqueue_all = [&]() -> int {
        if (pooled)
            HIP_TRY(hipEventRecord(ctx->ev_pool[ctx->ev_used - 2], st));
        if (in.timed)
            HIP_TRY(hipEventRecord(ctx->ev0, st));
        for (const plan::ScanLaunch& l : row_launches) {   // the rows with many pixels first
            ar.v0 = l.v0, ar.logical_blocks = l.logical_blocks, ar.per_xcd = l.per_xcd;
            if (int e = enqueue_scan(spr, ar, l.grid, ctx->stream_lds_bytes, st))
                return e;
        }
        for (const plan::ScanLaunch& l : launches) {
            a.v0 = l.v0, a.logical_blocks = l.logical_blocks, a.per_xcd = l.per_xcd;
            if (int e = enqueue_scan(sp, a, l.grid, ctx->stream_lds_bytes, st))
                return e;
        }
        if (in.timed) {
            HIP_TRY(hipEventRecord(ctx->ev1, st));
            ctx->ev_valid = true;
        }
        if (pooled)
            HIP_TRY(hipEventRecord(ctx->ev_pool[ctx->ev_used - 1], st));
        return RSLF_OK;
    };
    if (pooled)
        ctx->ev_used += 2;
    rc = enqueue_all();
    if (rc) {
        if (pooled)
            ctx->ev_used -= 2;
        return rc;
    }
    return stats ? read_stats(ctx, dim_d, stats) : RSLF_OK;
}

extern "C" int rslf_depth_epi_scan(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu,
                                   float dmin, float dmax, int dim_d, int s_hat, float* d_Ce_vu, uint8_t* d_Ce_mask_vu,
                                   float* d_Cd_vu, float* d_depth_vu, float* d_rbar_vu, const rslf_params* p,
                                   uint8_t* d_mask_vu, int32_t* d_idx_vu, float* d_score_vu, rslf_stats* stats) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    return depth_epi_scan(ctx, vol, d_dmin_vu, d_dmax_vu, dmin, dmax, dim_d, s_hat, d_Ce_vu, d_Ce_mask_vu, d_Cd_vu, d_depth_vu,
                          d_rbar_vu, p, d_mask_vu, d_idx_vu, d_score_vu, stats, scan_defaults(ctx));
}
RSLF_API_CATCH

// The sub-grid mode of the *_sub entries (include/rslf_hip.h).  The refinement reads the scan's arg-max and score planes: the
// caller's, or the context's own where the caller passes none.
static int subgrid_planes(rslf_ctx* ctx, const rslf_volume* vol, int subgrid, int32_t** idx, float** score)
{
    if (subgrid != 0 && subgrid != 1)
        return fail(RSLF_ERR_INVALID_ARG, "subgrid=%d: 0 or 1", subgrid);
    if (!subgrid)
        return RSLF_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n = (size_t)vol->V * vol->U;
    Scratch& sc = ctx->scratch;
    if (!*idx) {
        HIP_TRY(hip_err(sc.sub_idx.reserve(n * sizeof(int32_t))));
        *idx = sc.sub_idx.as<int32_t>();
    }
    if (!*score) {
        HIP_TRY(hip_err(sc.sub_score.reserve(n * sizeof(float))));
        *score = sc.sub_score.as<float>();
    }
    return RSLF_OK;
}

// depth_epi_scan, then with subgrid = 1 the refinement (k9_subgrid.hpp) of every pixel that received a disparity, in place on
// the depth plane.  subgrid = 0: depth_epi_scan's launches and nothing else.
static int depth_epi_scan_refined(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu, float dmin,
                                  float dmax, int dim_d, int s_hat, float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu,
                                  float* d_depth_vu, float* d_rbar_vu, const rslf_params* p, uint8_t* d_mask_vu, int32_t* d_idx_vu,
                                  float* d_score_vu, rslf_stats* stats, const ScanInputs& in, int subgrid)
{
    if (!ctx || !vol)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    int rc = subgrid_planes(ctx, vol, subgrid, &d_idx_vu, &d_score_vu);
    if (rc)
        return rc;
    rc = depth_epi_scan(ctx, vol, d_dmin_vu, d_dmax_vu, dmin, dmax, dim_d, s_hat, d_Ce_vu, d_Ce_mask_vu, d_Cd_vu, d_depth_vu, d_rbar_vu,
                        p, d_mask_vu, d_idx_vu, d_score_vu, subgrid ? nullptr : stats, in);
    if (rc || !subgrid)
        return rc;
    rc = subgrid_refine(ctx, vol, d_dmin_vu, d_dmax_vu, dmin, dmax, dim_d, s_hat, p, d_idx_vu, d_score_vu, d_depth_vu, nullptr, nullptr);
    if (rc)
        return rc;
    return stats ? read_stats(ctx, dim_d, stats) : RSLF_OK;
}

extern "C" int rslf_depth_epi_scan_sub(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu,
                                       float dmin, float dmax, int dim_d, int s_hat, float* d_Ce_vu, uint8_t* d_Ce_mask_vu,
                                       float* d_Cd_vu, float* d_depth_vu, float* d_rbar_vu, const rslf_params* p,
                                       uint8_t* d_mask_vu, int32_t* d_idx_vu, float* d_score_vu, rslf_stats* stats,
                                       int subgrid) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    return depth_epi_scan_refined(ctx, vol, d_dmin_vu, d_dmax_vu, dmin, dmax, dim_d, s_hat, d_Ce_vu, d_Ce_mask_vu, d_Cd_vu, d_depth_vu,
                                  d_rbar_vu, p, d_mask_vu, d_idx_vu, d_score_vu, stats, scan_defaults(ctx), subgrid);
}
RSLF_API_CATCH

extern "C" int rslf_kernel_columns_pile(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu,
                                        float dmin, float dmax, int dim_d, int s_hat, const rslf_params* p,
                                        const int32_t* d_idx_vu, float* d_K_vsu) RSLF_API_TRY
{
    if (!ctx || !vol || !d_idx_vu || !d_K_vsu)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    int rc = check_scan_args(vol, d_dmin_vu, d_dmax_vu, dim_d, s_hat, p);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    ScanArgs a = {};
    a.vol = view_of(vol);
    a.dmin_vu = d_dmin_vu;
    a.dmax_vu = d_dmax_vu;
    a.dmin = dmin;
    a.dmax = dmax;
    a.dim_d = dim_d;
    a.s_hat = s_hat;
    a.k = make_scan_consts(p);
    a.groups = 1;
    const dim3 grid((vol->U + 255) / 256, vol->V);
    if (vol->C == 1)
        hipLaunchKernelGGL(k2_kernel_column<1>, grid, dim3(256), 0, ctx->stream, a, d_idx_vu, d_K_vsu);
    else
        hipLaunchKernelGGL(k2_kernel_column<3>, grid, dim3(256), 0, ctx->stream, a, d_idx_vu, d_K_vsu);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}
RSLF_API_CATCH

static int depth_epi_pile(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu, float dmin,
                          float dmax, int dim_d, int s_hat, float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu, float* d_depth_vu,
                          float* d_rbar_vu, const rslf_params* p, uint8_t* d_mask_vu, int32_t* d_idx_vu, float* d_score_vu,
                          float* d_depth_raw_vu, rslf_stats* stats, const ScanInputs& in, int subgrid = 0)
{
    if (!ctx || !vol || !d_depth_vu)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = ensure_plane_scratch(ctx, vol->V, vol->U);
    if (rc)
        return rc;
    const size_t n = (size_t)vol->V * vol->U;
    hipStream_t st = ctx->stream;
    // core.hpp:799-854: the scan of every EPI writes the RAW disparities -- into the caller's raw plane if one is
    // wanted (over the zeros best_depth starts from, dc.hpp:507), else into scratch, where no background is needed:
    // the median reads the raw plane at mask pixels only, and every mask pixel has been written by the scan ...
    // With a caller's scan mask, mask pixels that are NOT scanned now keep the disparity the plane came in with
    // (a_best_depth_v_u is in/out, core.hpp:305), and the median reads them: the raw plane then starts as a copy.
    float* raw = d_depth_raw_vu ? d_depth_raw_vu : ctx->scratch.depth_tmp.as<float>();
    if (d_mask_vu)
        HIP_TRY(hipMemcpyAsync(raw, d_depth_vu, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    else if (d_depth_raw_vu)
        HIP_TRY(hipMemsetAsync(d_depth_raw_vu, 0, n * sizeof(float), st));
    // (subgrid = 1: every disparity the scan wrote is then moved off the grid, in place -- the median filters refined values)
    rc = depth_epi_scan_refined(ctx, vol, d_dmin_vu, d_dmax_vu, dmin, dmax, dim_d, s_hat, d_Ce_vu, d_Ce_mask_vu, d_Cd_vu, raw, d_rbar_vu,
                                p, d_mask_vu, d_idx_vu, d_score_vu, nullptr, in, subgrid);
    if (rc)
        return rc;
    // ... then core.hpp:881-892: median over the EDGE mask, result replaces best_depth -- written straight into the
    // caller's plane (every pixel: 0 where the mask is 0, core.hpp:678-679), so no plane is copied
    rc = rslf_selective_median(ctx, vol, raw, d_depth_vu, s_hat, p->median_filter_size, d_Ce_mask_vu, p->median_filter_epsilon);
    if (rc)
        return rc;
    return stats ? read_stats(ctx, dim_d, stats) : RSLF_OK;
}

extern "C" int rslf_depth_epi_pile(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu,
                                   float dmin, float dmax, int dim_d, int s_hat, float* d_Ce_vu, uint8_t* d_Ce_mask_vu,
                                   float* d_Cd_vu, float* d_depth_vu, float* d_rbar_vu, const rslf_params* p,
                                   uint8_t* d_mask_vu, int32_t* d_idx_vu, float* d_score_vu, float* d_depth_raw_vu,
                                   rslf_stats* stats) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    return depth_epi_pile(ctx, vol, d_dmin_vu, d_dmax_vu, dmin, dmax, dim_d, s_hat, d_Ce_vu, d_Ce_mask_vu, d_Cd_vu, d_depth_vu,
                          d_rbar_vu, p, d_mask_vu, d_idx_vu, d_score_vu, d_depth_raw_vu, stats, scan_defaults(ctx));
}
RSLF_API_CATCH

extern "C" int rslf_depth_epi_pile_sub(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu,
                                       float dmin, float dmax, int dim_d, int s_hat, float* d_Ce_vu, uint8_t* d_Ce_mask_vu,
                                       float* d_Cd_vu, float* d_depth_vu, float* d_rbar_vu, const rslf_params* p,
                                       uint8_t* d_mask_vu, int32_t* d_idx_vu, float* d_score_vu, float* d_depth_raw_vu,
                                       rslf_stats* stats, int subgrid) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    return depth_epi_pile(ctx, vol, d_dmin_vu, d_dmax_vu, dmin, dmax, dim_d, s_hat, d_Ce_vu, d_Ce_mask_vu, d_Cd_vu, d_depth_vu,
                          d_rbar_vu, p, d_mask_vu, d_idx_vu, d_score_vu, d_depth_raw_vu, stats, scan_defaults(ctx), subgrid);
}
RSLF_API_CATCH

// rslf_depth1d_pile_run and its _sub form
static int depth1d_pile_run(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, int s_hat,
                            const rslf_params* p, float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu, float* d_depth_vu,
                            float* d_rbar_vu, int32_t* d_idx_vu, float* d_score_vu, float* d_depth_raw_vu, rslf_stats* stats,
                            int subgrid)
{
    if (!ctx || !vol || !d_Ce_vu || !d_Ce_mask_vu || !d_Cd_vu || !d_depth_vu || !d_rbar_vu)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (subgrid != 0 && subgrid != 1)
        return fail(RSLF_ERR_INVALID_ARG, "subgrid=%d: 0 or 1", subgrid);
    HIP_TRY(hipSetDevice(ctx->device));
    s_hat = plan::resolve_s_hat(s_hat, vol->S);
    const size_t n = (size_t)vol->V * vol->U;
    hipStream_t st = ctx->stream;
    // dc.hpp:501-510 (C_e and C_d are uninitialised there; zero is the intended start)
    HIP_TRY(hipMemsetAsync(d_Ce_vu, 0, n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(d_Cd_vu, 0, n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(d_depth_vu, 0, n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(d_rbar_vu, 0, n * vol->C * sizeof(float), st));
    int rc = check_params(p);
    if (rc)
        return rc;
    // dc.hpp:538 + the findNonZero of dc.hpp:547's callee (core.hpp:513-516) in ONE launch when nothing sits between
    // them (plan::fuse_k1_compaction).  A pile step is then three launches -- edge confidence + compaction, scan, selective
    // median -- and no plane is copied.
    ScanInputs in = scan_defaults(ctx);
    if (vol->filled && plan::fuse_k1_compaction(p->edge_confidence_opening_size, ctx->force_packed, n)) {
        rc = ensure_plane_scratch(ctx, vol->V, vol->U);
        if (rc)
            return rc;
        const Scratch& sc = ctx->scratch;
        EdgeConsts ec;
        ec.filter_size = p->edge_confidence_filter_size;
        ec.cut_shadows = p->cut_shadows;
        ec.shadow_level = p->shadow_level;
        ec.edge_thr = p->edge_score_threshold;
        if (in.zero_total)
            HIP_TRY(hipMemsetAsync(sc.pixel_total(), 0, sizeof(unsigned long long), st));
        if (vol->C == 1)
            hipLaunchKernelGGL(k1_edge_confidence_compact<1>, dim3(vol->V), dim3(256), 0, st, view_of(vol), s_hat, ec, d_Ce_vu,
                               d_Ce_mask_vu, sc.list.as<int>(), sc.count.as<int>(), sc.pixel_total());
        else
            hipLaunchKernelGGL(k1_edge_confidence_compact<3>, dim3(vol->V), dim3(256), 0, st, view_of(vol), s_hat, ec, d_Ce_vu,
                               d_Ce_mask_vu, sc.list.as<int>(), sc.count.as<int>(), sc.pixel_total());
        HIP_TRY(hipGetLastError());
        in.lists = ScanInputs::kRowLists;
    } else {
        rc = rslf_edge_confidence_pile(ctx, vol, s_hat, p, d_Ce_vu, d_Ce_mask_vu);   // dc.hpp:538
        if (rc)
            return rc;
    }
    return depth_epi_pile(ctx, vol, nullptr, nullptr, dmin, dmax, dim_d, s_hat, d_Ce_vu, d_Ce_mask_vu, d_Cd_vu, d_depth_vu,   // dc.hpp:547
                          d_rbar_vu, p, nullptr, d_idx_vu, d_score_vu, d_depth_raw_vu, stats, in, subgrid);
}

extern "C" int rslf_depth1d_pile_run(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, int s_hat,
                                     const rslf_params* p, float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu,
                                     float* d_depth_vu, float* d_rbar_vu, int32_t* d_idx_vu, float* d_score_vu,
                                     float* d_depth_raw_vu, rslf_stats* stats) RSLF_API_TRY
{
    return depth1d_pile_run(ctx, vol, dmin, dmax, dim_d, s_hat, p, d_Ce_vu, d_Ce_mask_vu, d_Cd_vu, d_depth_vu, d_rbar_vu, d_idx_vu,
                            d_score_vu, d_depth_raw_vu, stats, 0);
}
RSLF_API_CATCH

extern "C" int rslf_depth1d_pile_run_sub(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, int s_hat,
                                         const rslf_params* p, float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu,
                                         float* d_depth_vu, float* d_rbar_vu, int32_t* d_idx_vu, float* d_score_vu,
                                         float* d_depth_raw_vu, rslf_stats* stats, int subgrid) RSLF_API_TRY
{
    return depth1d_pile_run(ctx, vol, dmin, dmax, dim_d, s_hat, p, d_Ce_vu, d_Ce_mask_vu, d_Cd_vu, d_depth_vu, d_rbar_vu, d_idx_vu,
                            d_score_vu, d_depth_raw_vu, stats, subgrid);
}
RSLF_API_CATCH

// rslf_depth1d_run and its _sub form
static int depth1d_run(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, int s_hat, const rslf_params* p,
                       float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu, float* d_depth_vu, float* d_rbar_vu, int32_t* d_idx_vu,
                       float* d_score_vu, rslf_stats* stats, int subgrid)
{
    if (!ctx || !vol || !d_Ce_vu || !d_Ce_mask_vu || !d_Cd_vu || !d_depth_vu || !d_rbar_vu)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    s_hat = plan::resolve_s_hat(s_hat, vol->S);   // dc.hpp:303-311
    const size_t n = (size_t)vol->V * vol->U;
    hipStream_t st = ctx->stream;
    // dc.hpp:313-322: zero-initialised outputs
    HIP_TRY(hipMemsetAsync(d_Ce_vu, 0, n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(d_Cd_vu, 0, n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(d_depth_vu, 0, n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(d_rbar_vu, 0, n * vol->C * sizeof(float), st));
    int rc = rslf_edge_confidence_pile(ctx, vol, s_hat, p, d_Ce_vu, d_Ce_mask_vu);   // dc.hpp:347
    if (rc)
        return rc;
    return depth_epi_scan_refined(ctx, vol, nullptr, nullptr, dmin, dmax, dim_d, s_hat, d_Ce_vu, d_Ce_mask_vu, d_Cd_vu, d_depth_vu,   // dc.hpp:356
                                  d_rbar_vu, p, nullptr, d_idx_vu, d_score_vu, stats, scan_defaults(ctx), subgrid);
}

extern "C" int rslf_depth1d_run(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, int s_hat,
                                const rslf_params* p, float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu, float* d_depth_vu,
                                float* d_rbar_vu, int32_t* d_idx_vu, float* d_score_vu, rslf_stats* stats) RSLF_API_TRY
{
    return depth1d_run(ctx, vol, dmin, dmax, dim_d, s_hat, p, d_Ce_vu, d_Ce_mask_vu, d_Cd_vu, d_depth_vu, d_rbar_vu, d_idx_vu, d_score_vu,
                       stats, 0);
}
RSLF_API_CATCH

extern "C" int rslf_depth1d_run_sub(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, int s_hat,
                                    const rslf_params* p, float* d_Ce_vu, uint8_t* d_Ce_mask_vu, float* d_Cd_vu, float* d_depth_vu,
                                    float* d_rbar_vu, int32_t* d_idx_vu, float* d_score_vu, rslf_stats* stats,
                                    int subgrid) RSLF_API_TRY
{
    return depth1d_run(ctx, vol, dmin, dmax, dim_d, s_hat, p, d_Ce_vu, d_Ce_mask_vu, d_Cd_vu, d_depth_vu, d_rbar_vu, d_idx_vu, d_score_vu,
                       stats, subgrid);
}
RSLF_API_CATCH

// rslf_depth1d_pile_run_host and its _sub form
static int depth1d_pile_run_host(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, int s_hat,
                                 const rslf_params* p, float* h_Ce_vu, uint8_t* h_Ce_mask_vu, float* h_Cd_vu, float* h_depth_vu,
                                 float* h_rbar_vu, int32_t* h_idx_vu, float* h_score_vu, float* h_depth_raw_vu, rslf_stats* stats,
                                 int subgrid)
{
    if (!ctx || !vol)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n = (size_t)vol->V * vol->U;
    const size_t bytes = plan::plane_layout(n, vol->C, 0).bytes;   // one device block for the eight planes
    DevBuf blk;   // (freed when the call returns, however it returns)
    hipError_t e = blk.alloc(bytes);
    if (e != hipSuccess)
        return fail(RSLF_ERR_ALLOC, "hipMalloc(%zu) for result planes failed: %s", bytes, hipGetErrorString(e));
    const plan::PilePlanes q = plan::carve(blk.as<char>(), n, vol->C);
    plan::PilePlanes out;
    out.Ce = h_Ce_vu, out.mask = h_Ce_mask_vu, out.Cd = h_Cd_vu, out.depth = h_depth_vu, out.rbar = h_rbar_vu, out.idx = h_idx_vu;
    out.score = h_score_vu, out.raw = h_depth_raw_vu;
    int rc = depth1d_pile_run(ctx, vol, dmin, dmax, dim_d, s_hat, p, q.Ce, q.mask, q.Cd, q.depth, q.rbar, q.idx, q.score, q.raw, nullptr,
                              subgrid);
    hipStream_t st = ctx->stream;
    if (rc == RSLF_OK) {
        hipError_t ce = (hipError_t)plan::for_each_plane(out, q, vol->C, [&](void* h, const void* d, size_t bpp) {
            return (int)hipMemcpyAsync(h, d, n * bpp, hipMemcpyDeviceToHost, st);
        });
        if (ce == hipSuccess) ce = hipStreamSynchronize(st);
        if (ce != hipSuccess)
            rc = fail(RSLF_ERR_HIP, "result download failed: %s", hipGetErrorString(ce));
    } else {
        (void)hipStreamSynchronize(st);
    }
    if (rc == RSLF_OK && stats) {
        unsigned long long tot = 0;
        if (hipMemcpy(&tot, ctx->scratch.pixel_total(), sizeof(tot), hipMemcpyDeviceToHost) == hipSuccess)
            fill_stats(ctx, tot, dim_d, stats);
    }
    return rc;
}

extern "C" int rslf_depth1d_pile_run_host(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, int s_hat,
                                          const rslf_params* p, float* h_Ce_vu, uint8_t* h_Ce_mask_vu, float* h_Cd_vu,
                                          float* h_depth_vu, float* h_rbar_vu, int32_t* h_idx_vu, float* h_score_vu,
                                          float* h_depth_raw_vu, rslf_stats* stats) RSLF_API_TRY
{
    return depth1d_pile_run_host(ctx, vol, dmin, dmax, dim_d, s_hat, p, h_Ce_vu, h_Ce_mask_vu, h_Cd_vu, h_depth_vu, h_rbar_vu, h_idx_vu,
                                 h_score_vu, h_depth_raw_vu, stats, 0);
}
RSLF_API_CATCH

extern "C" int rslf_depth1d_pile_run_host_sub(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, int s_hat,
                                              const rslf_params* p, float* h_Ce_vu, uint8_t* h_Ce_mask_vu, float* h_Cd_vu,
                                              float* h_depth_vu, float* h_rbar_vu, int32_t* h_idx_vu, float* h_score_vu,
                                              float* h_depth_raw_vu, rslf_stats* stats, int subgrid) RSLF_API_TRY
{
    return depth1d_pile_run_host(ctx, vol, dmin, dmax, dim_d, s_hat, p, h_Ce_vu, h_Ce_mask_vu, h_Cd_vu, h_depth_vu, h_rbar_vu, h_idx_vu,
                                 h_score_vu, h_depth_raw_vu, stats, subgrid);
}
RSLF_API_CATCH

extern "C" int rslf_scan_time_total_ms(rslf_ctx* ctx, float* ms, int* launches) RSLF_API_TRY
{
    if (!ctx || !ms)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    double sum = 0.0;
    for (size_t i = 0; i + 1 < ctx->ev_used; i += 2) {
        float t = 0.0f;
        HIP_TRY(hipEventSynchronize(ctx->ev_pool[i + 1]));
        HIP_TRY(hipEventElapsedTime(&t, ctx->ev_pool[i], ctx->ev_pool[i + 1]));
        sum += (double)t;
    }
    *ms = (float)sum;
    if (launches)
        *launches = (int)(ctx->ev_used / 2);
    ctx->ev_used = 0;
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_last_scan_row_exact(rslf_ctx* ctx, int* attached, int* exact_hypotheses) RSLF_API_TRY
{
    if (!ctx || !attached || !exact_hypotheses)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    *attached = ctx->last_row_exact ? 1 : 0;
    *exact_hypotheses = 0;
    if (!ctx->last_row_exact)
        return RSLF_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const RowExactKey& k = ctx->row_exact_key;   // (the last launch's: attach_row_exact left it there)
    std::vector<int> flags((size_t)k.dim_d);
    const char* d_flags = ctx->scratch.row_exact.as<char>() + (size_t)k.dim_d * ((size_t)k.slots * 16 + sizeof(float));
    HIP_TRY(hipMemcpyAsync(flags.data(), d_flags, flags.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int f : flags)
        *exact_hypotheses += f != 0;
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_last_scan_kernel_ms(rslf_ctx* ctx, float* ms) RSLF_API_TRY
{
    if (!ctx || !ms)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (!ctx->ev_valid)
        return fail(RSLF_ERR_INVALID_ARG, "no scan kernel has been launched on this context");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventSynchronize(ctx->ev1));
    HIP_TRY(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return RSLF_OK;
}
RSLF_API_CATCH
