// librslf_hip.so: the 2-D sweep (Depth2DComputer::run, core.hpp:901-1133) -- one visit per view, scan (unit 2),
// selective median + claims, apply + the next visit's compaction (K4), and the sweep's line confidence (K7).  The peaks mode's
// step is rslf_sweep_peaks.hip's.  C-ABI: include/rslf_hip.h.
#include "rslf_internal.hpp"
#include "rslf_plan_subgrid.hpp"
#include "rslf_plan_sweep_gate.hpp"
#include "rslf_plan_sweep_peaks.hpp"

#include <algorithm>
#include <cmath>

#include "k3_median.hpp"
#include "k4_propagate.hpp"
#include "k7_line_conf.hpp"

using namespace rslf;

// ---- "next" row: the 2-D sweep ----------------------------------------------

// Every buffer has its own capacity: winner / running mask hold S*V*U entries, the flags S*V*ceil(U/256), the median plane
// V*U.  (A single S*V*U capacity once let a later volume with fewer views but larger planes overrun the plane: found by
// tools/fuzz_sweep.py.)
static int ensure_sweep_scratch(rslf_ctx* ctx, const rslf_volume* vol)
{
    Scratch& sc = ctx->scratch;
    const size_t n = (size_t)vol->S * vol->V * vol->U;
    const Reserved w = sc.winner.reserve(n * sizeof(int));
    HIP_TRY(hip_err(w));
    if (w.fresh)   // every claim pass is undone by its apply pass, so one fill lasts
        HIP_TRY(hipMemsetAsync(sc.winner.get(), 0x7F, sc.winner.capacity(), ctx->stream));
    HIP_TRY(hip_err(sc.sweep_mask.reserve(n)));
    const size_t flags = (size_t)vol->S * vol->V * ((vol->U + 255) / 256);
    HIP_TRY(hip_err(sc.remain.reserve(flags * sizeof(int))));
    const Reserved d = sc.dirty.reserve(flags);
    HIP_TRY(hip_err(d));
    if (d.fresh)   // every apply pass leaves them at 0 again
        HIP_TRY(hipMemsetAsync(sc.dirty.get(), 0, sc.dirty.capacity(), ctx->stream));
    HIP_TRY(hip_err(sc.filtered.reserve((size_t)vol->V * vol->U * sizeof(float))));
    return RSLF_OK;
}

// The sweep one visit at a time (rslf_sweep_*), and rslf_depth_epi_2d on top of it.  rslf_sweep_end closes it; after an
// error the winners are refilled on the next sweep (a claim pass whose apply never ran leaves them set).
// The order of the visits (core.hpp:981-990): plan::sweep_order.
static void sweep_close(rslf_ctx* ctx, bool ok)
{
    ctx->last_gated = ok && ctx->sweep.prop_ratio > 0.0f;   // the count rslf_sweep_withheld reports; 0 for any other sweep
    ctx->sweep = SweepState();   // line confidence too is state of ONE sweep (rslf_sweep_line_confidence)
    if (!ok) {
        ctx->scratch.winner.mark_stale();   // claims without their apply pass may be left behind: fresh winners and flags next time
        ctx->scratch.dirty.mark_stale();
    }
}

// What a visit's scan is given.  After the centre view, propagation has explained most pixels: a visit scans a few per
// scanline.  They go in one packed list -- the one the previous visit's apply pass made, if it made one -- and each tile's
// hypotheses are shared out over up to kSweepGroups workgroups (k2_scan.hpp).  The visits sum their pixels; the first is timed.
static ScanInputs visit_inputs(bool first, bool listed)
{
    ScanInputs in;
    in.zero_total = false;
    in.timed = first;
    if (!first) {
        in.groups = plan::kSweepGroups;
        in.packed = true;
        in.lists = listed ? ScanInputs::kPackedList : ScanInputs::kCompact;
        in.packed_n_zero = !listed;   // k34_median_claim zeroed the length; a listing apply pass set it again
    }
    return in;
}

extern "C" int rslf_sweep_begin(rslf_ctx* ctx, const rslf_volume* vol, const uint8_t* d_Ce_mask_svu, uint8_t* d_scan_mask_svu,
                                int dim_d, int v_lo, int v_hi) RSLF_API_TRY
{
    if (!ctx || !vol || !d_Ce_mask_svu)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (v_lo < 0 || v_hi > vol->V || v_lo >= v_hi)
        return fail(RSLF_ERR_INVALID_ARG, "active scanlines [%d, %d) outside the volume's %d", v_lo, v_hi, vol->V);
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->sweep.open)
        sweep_close(ctx, false);   // a sweep left open by a caller's error path
    int rc = ensure_sweep_scratch(ctx, vol);
    if (rc)
        return rc;
    const int S = vol->S, V = vol->V, U = vol->U;
    const size_t n = (size_t)V * U;
    hipStream_t st = ctx->stream;
    uint8_t* mask_svu = d_scan_mask_svu ? d_scan_mask_svu : ctx->scratch.sweep_mask.as<uint8_t>();
    // core.hpp:958-965: running masks start as clones of the edge masks ...
    HIP_TRY(hipMemcpyAsync(mask_svu, d_Ce_mask_svu, (size_t)S * n, hipMemcpyDeviceToDevice, st));
    // ... except on halo scanlines (a sharded sweep): never scanned, never painted here -- their owner does both
    if (v_lo > 0)
        HIP_TRY(hipMemset2DAsync(mask_svu, n, 0, (size_t)v_lo * U, S, st));
    if (v_hi < V)
        HIP_TRY(hipMemset2DAsync(mask_svu + (size_t)v_hi * U, n, 0, (size_t)(V - v_hi) * U, S, st));
    HIP_TRY(hipMemsetAsync(ctx->scratch.pixel_total(), 0, sizeof(unsigned long long), st));
    {   // pixels of the running masks per 256-column segment: what lets the claims of the later visits skip most views
        const long long rows = (long long)S * V;
        const long long items = rows * ((U + 255) / 256);
        if (items > (1ll << 31) - 1)
            return fail(RSLF_ERR_UNSUPPORTED, "%d views x %d scanlines x %d columns: too large for one counting launch", S, V, U);
        hipLaunchKernelGGL(k4_count_segments, dim3((unsigned)items), dim3(256), 0, st, mask_svu, rows, U, ctx->scratch.remain.as<int>());
        HIP_TRY(hipGetLastError());
    }
    // the sparse visits' records, sized before the first visit (no allocation in the middle of the sequence; should a
    // visit ask for more -- nearest-neighbour interpolation -- it sizes them itself)
    rc = sweep_scan_presize(ctx, vol, dim_d, visit_inputs(false, true));
    if (rc)
        return rc;
    SweepState sw;   // first visit next, nothing scanned or listed, no line confidence
    sw.open = true;
    sw.keep_total = true;
    sw.mask_run = mask_svu;
    sw.expect = plan::sweep_order(S)[0];
    sw.dim_d = dim_d;
    ctx->sweep = sw;
    return RSLF_OK;
}
RSLF_API_CATCH

// ---- line confidence (K7; core.hpp:1032-1081 under _USE_LINE_CONFIDENCE_SCORE) ---------------------------------------

// One K7 launch.  idx_vu (nullable): the visit's arg-max plane, with which `a` holds the scan's arguments and C its channels.
static int launch_line_confidence(rslf_ctx* ctx, const LineConfArgs& q, const ScanArgs& a, const int32_t* idx_vu, int C)
{
    if (q.V > 65535 || q.U > (1 << 24))
        return fail(RSLF_ERR_UNSUPPORTED, "%d scanlines x %d columns: too large for one line-confidence launch", q.V, q.U);
    const dim3 grid((q.U + 255) / 256, q.V);
    if (C == 3)
        hipLaunchKernelGGL(k7_line_confidence<3>, grid, dim3(256), 0, ctx->stream, q, a, idx_vu);
    else
        hipLaunchKernelGGL(k7_line_confidence<1>, grid, dim3(256), 0, ctx->stream, q, a, idx_vu);
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

// core.hpp:1054-1079 on caller planes (include/rslf_hip.h)
extern "C" int rslf_line_confidence_pile(rslf_ctx* ctx, int V, int S, int U, int s_hat, const float* d_Ce_svu, const float* d_K_vsu,
                                         const float* d_depth_vu, const uint8_t* d_Ce_mask_vu, float* d_Cl_vu) RSLF_API_TRY
{
    if (!ctx || !d_Ce_svu || !d_K_vsu || !d_depth_vu || !d_Ce_mask_vu || !d_Cl_vu)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (V < 1 || S < 1 || U < 1)
        return fail(RSLF_ERR_INVALID_ARG, "V=%d S=%d U=%d: every dimension must be positive", V, S, U);
    if (s_hat < 0 || s_hat >= S)
        return fail(RSLF_ERR_INVALID_ARG, "s_hat=%d outside [0,%d)", s_hat, S);
    HIP_TRY(hipSetDevice(ctx->device));
    LineConfArgs q = {};
    q.V = V, q.S = S, q.U = U, q.s_hat = s_hat;
    q.Ce_svu = d_Ce_svu;
    q.K_vsu = const_cast<float*>(d_K_vsu);   // written only with an arg-max plane: there is none here
    q.depth_vu = d_depth_vu;
    q.mask_vu = d_Ce_mask_vu;
    q.Cl_vu = d_Cl_vu;
    return launch_line_confidence(ctx, q, ScanArgs{}, nullptr, 1);
}
RSLF_API_CATCH

// A line mode that is none, or one that lacks its plane
static int line_conf_refusal(int mode, const float* Cl_svu)
{
    if (!plan::line_conf_mode_ok(mode))
        return fail(RSLF_ERR_INVALID_ARG, "line confidence mode %d: must be RSLF_LINE_CONF_OFF, _AS_BUILT or _GATE", mode);
    if (mode != RSLF_LINE_CONF_OFF && !Cl_svu)
        return fail(RSLF_ERR_INVALID_ARG, "line confidence mode %d needs the [S][V][U] plane", mode);
    return RSLF_OK;
}

// dc.hpp:721-738, :791-792 and core.hpp:975-979: the planes a sweep with line confidence keeps (include/rslf_hip.h)
extern "C" int rslf_sweep_line_confidence(rslf_ctx* ctx, const rslf_volume* vol, int mode, float* d_Cl_svu) RSLF_API_TRY
{
    if (!ctx || !vol)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (int rc = line_conf_refusal(mode, d_Cl_svu))
        return rc;
    SweepState& sw = ctx->sweep;
    if (!sw.open || sw.scanned || !sw.first)
        return fail(RSLF_ERR_INVALID_ARG, "rslf_sweep_line_confidence belongs between rslf_sweep_begin and the first visit");
    HIP_TRY(hipSetDevice(ctx->device));
    sw.lc_mode = RSLF_LINE_CONF_OFF;
    sw.lc_Cl_svu = nullptr;
    if (mode == RSLF_LINE_CONF_OFF) {
        if (sw.subgrid || sw.peaks)   // line confidence switched off again after rslf_sweep_subgrid / _peaks: the visits need an arg-max plane of their own
            HIP_TRY(hip_err(ctx->scratch.sub_idx.reserve(plan::sweep_subgrid_plane_bytes(true, vol->V, vol->U))));
        return RSLF_OK;
    }
    // buffers of their own, not shared ones: they are held until rslf_sweep_end
    Scratch& sc = ctx->scratch;
    const size_t kb = plan::line_conf_columns_bytes(mode, vol->V, vol->S, vol->U);
    HIP_TRY(hip_err(sc.lc_columns.reserve(kb)));
    HIP_TRY(hip_err(sc.lc_argmax.reserve(plan::line_conf_argmax_bytes(mode, vol->V, vol->U))));
    // core.hpp:975-979 leaves K uninitialised; here a column nobody has written reads as zeros.  The arg-max
    // plane is refilled with -1 by every scan.
    HIP_TRY(hipMemsetAsync(sc.lc_columns.get(), 0, kb, ctx->stream));
    sw.lc_K_vsu = sc.lc_columns.as<float>();
    sw.lc_idx_vu = sc.lc_argmax.as<int32_t>();
    sw.lc_Cl_svu = d_Cl_svu;
    sw.lc_mode = mode;
    return RSLF_OK;
}
RSLF_API_CATCH

// The sub-grid mode of an open sweep (include/rslf_hip.h; k9_subgrid.hpp): every visit's scan keeps its arg max and the
// winner's score, and the refinement follows the scan in place on the view's raw depth plane.
extern "C" int rslf_sweep_subgrid(rslf_ctx* ctx, const rslf_volume* vol, int on) RSLF_API_TRY
{
    if (!ctx || !vol)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (on != 0 && on != 1)
        return fail(RSLF_ERR_INVALID_ARG, "rslf_sweep_subgrid: on=%d: 0 or 1", on);
    SweepState& sw = ctx->sweep;
    if (!sw.open || sw.scanned || !sw.first)
        return fail(RSLF_ERR_INVALID_ARG, "rslf_sweep_subgrid belongs between rslf_sweep_begin and the first visit");
    HIP_TRY(hipSetDevice(ctx->device));
    sw.subgrid = false;
    if (!on)
        return RSLF_OK;
    // sized here, never inside a visit; held until rslf_sweep_end (buffers of the context's own, not shared ones).  With line
    // confidence on, the visits' arg-max plane is K7's: no second one (the two setters come in either order)
    Scratch& sc = ctx->scratch;
    const size_t bytes = plan::sweep_subgrid_plane_bytes(true, vol->V, vol->U);
    if (sw.lc_mode == RSLF_LINE_CONF_OFF)
        HIP_TRY(hip_err(sc.sub_idx.reserve(bytes)));
    HIP_TRY(hip_err(sc.sub_score.reserve(bytes)));
    sw.subgrid = true;
    return RSLF_OK;
}
RSLF_API_CATCH

// The gate by peak ratio of an open sweep in the peaks mode (include/rslf_hip.h; k4_propagate.hpp, ClaimGate): every visit's
// claims come from k34_median_claim_gated.  The refusals: plan::sweep_gate_args.
static int gate_refusal(plan::SweepGateArg why, float ratio, const char* who)
{
    switch (why) {
    case plan::kSweepGateOk:
        return RSLF_OK;
    case plan::kSweepGateBadRatio:
        return fail(RSLF_ERR_INVALID_ARG, "%s: propagation_ratio=%g: 0 (off) or a ratio in (0, 1]", who, (double)ratio);
    case plan::kSweepGateWindow:
        return fail(RSLF_ERR_INVALID_ARG, "%s belongs between rslf_sweep_peaks and the first visit", who);
    case plan::kSweepGateNoPeaks:
        return fail(RSLF_ERR_INVALID_ARG, "%s: propagation_ratio=%g reads the peak planes: it needs the peaks mode (rslf_sweep_peaks)", who,
                    (double)ratio);
    case plan::kSweepGateNullPlane:
        return fail(RSLF_ERR_INVALID_ARG, "%s: propagation_ratio=%g needs all four peak planes, and one is NULL", who, (double)ratio);
    }
    return fail(RSLF_ERR_INTERNAL, "%s: unknown refusal", who);
}

extern "C" int rslf_sweep_propagation_ratio(rslf_ctx* ctx, const rslf_volume* vol, float ratio) RSLF_API_TRY
{
    if (!ctx || !vol)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    SweepState& sw = ctx->sweep;
    const rslf_peaks& pk = sw.pk;
    if (int rc = gate_refusal(plan::sweep_gate_args(ratio, sw.open, sw.scanned, sw.first, sw.peaks, pk.idx != nullptr, pk.score != nullptr,
                                                    pk.runner_idx != nullptr, pk.runner_score != nullptr),
                              ratio, "rslf_sweep_propagation_ratio"))
        return rc;
    sw.prop_ratio = 0.0f;
    if (!plan::sweep_gate_on(ratio))
        return RSLF_OK;
    // sized here, never inside a visit; the count starts at 0 in stream order, ahead of the first visit's claims
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hip_err(ctx->scratch.withheld.reserve(plan::sweep_gate_counter_bytes(ratio))));
    HIP_TRY(hipMemsetAsync(ctx->scratch.withheld.get(), 0, sizeof(unsigned long long), ctx->stream));
    sw.prop_ratio = ratio;
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_sweep_withheld(rslf_ctx* ctx, unsigned long long* n) RSLF_API_TRY
{
    if (!ctx || !n)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (ctx->sweep.open)
        return fail(RSLF_ERR_INVALID_ARG, "rslf_sweep_withheld reports an ended sweep: call it after rslf_sweep_end");
    HIP_TRY(hipSetDevice(ctx->device));
    *n = 0;
    if (ctx->last_gated)
        HIP_TRY(hipMemcpyAsync(n, ctx->scratch.withheld.get(), sizeof(*n), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_sweep_visit_scan(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu,
                                     float dmin, float dmax, int dim_d, int s_hat, float* d_Ce_svu, uint8_t* d_Ce_mask_svu,
                                     float* d_Cd_svu, float* d_depth_svu, float* d_rbar_svu, const rslf_params* p) RSLF_API_TRY
{
    if (!ctx || !vol || !d_Ce_svu || !d_Ce_mask_svu || !d_Cd_svu || !d_depth_svu || !d_rbar_svu)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (!ctx->sweep.open)
        return fail(RSLF_ERR_INVALID_ARG, "rslf_sweep_visit_scan without rslf_sweep_begin");
    if ((d_dmin_svu == nullptr) != (d_dmax_svu == nullptr))
        return fail(RSLF_ERR_INVALID_ARG, "d_dmin_svu and d_dmax_svu must both be given or both be NULL");
    if (s_hat < 0 || s_hat >= vol->S)
        return fail(RSLF_ERR_INVALID_ARG, "s_hat=%d outside [0,%d)", s_hat, vol->S);
    if (s_hat != ctx->sweep.expect)   // the previous visit has already listed this view's pixels (k4_propagate_apply)
        return fail(RSLF_ERR_INVALID_ARG, "the sweep visits view %d next (core.hpp:981-990), not %d", ctx->sweep.expect, s_hat);
    const size_t n = (size_t)vol->V * vol->U;
    // core.hpp:1012-1028: the pile call is the scan of every EPI followed by the selective median.  In the
    // reference the stored plane keeps the RAW depths and only the local header is rebound to the median
    // (core.hpp:892), which the propagation then paints from: so the scan writes the view's depth plane and the median
    // goes to Scratch::filtered (rslf_sweep_visit_finish) -- no plane copies.
    ctx->sweep.scanned = true;
    const bool lc = ctx->sweep.lc_mode != RSLF_LINE_CONF_OFF;   // K7 re-runs the winners: the scan keeps its arg-max indices
    // Sub-grid mode: the scan also keeps the winner's score, and K9 follows it.  Which form is decided before the scan so
    // that nothing below can fail between the two; one arg-max plane serves K7 and K9.
    const plan::SubgridForm form = plan::sweep_subgrid_form(ctx->sweep.subgrid, ctx->sweep.first, ctx->sweep.listed,
                                                            ctx->subgrid_list, (long long)n);
    const float* dmin_vu = d_dmin_svu ? d_dmin_svu + (size_t)s_hat * n : nullptr;
    const float* dmax_vu = d_dmax_svu ? d_dmax_svu + (size_t)s_hat * n : nullptr;
    // Peaks mode: the step follows the refinement; it reads the same arg-max plane (one for all three modes).
    const plan::PeaksForm pk_form = plan::sweep_peaks_form(ctx->sweep.peaks, ctx->sweep.first, ctx->sweep.listed, ctx->peaks_list,
                                                           (long long)n);
    const bool keep = form != plan::kSubgridNone || pk_form != plan::kPeaksNone;
    int32_t* idx_vu = lc ? ctx->sweep.lc_idx_vu : keep ? ctx->scratch.sub_idx.as<int32_t>() : nullptr;
    float* score_vu = keep ? ctx->scratch.sub_score.as<float>() : nullptr;
    ScanInputs in = visit_inputs(ctx->sweep.first, ctx->sweep.listed);
    in.clear_score = false;   // K9 reads a score only where this scan wrote idx >= 0, and so the score: one fill less a visit
    int rc = depth_epi_scan(ctx, vol, dmin_vu, dmax_vu, dmin, dmax, dim_d, s_hat, d_Ce_svu + (size_t)s_hat * n,
                            d_Ce_mask_svu + (size_t)s_hat * n, d_Cd_svu + (size_t)s_hat * n, d_depth_svu + (size_t)s_hat * n,
                            d_rbar_svu + (size_t)s_hat * n * vol->C, p, ctx->sweep.mask_run + (size_t)s_hat * n, idx_vu, score_vu,
                            nullptr, in);
    // The refinement, queued here: before k34_median_claim (or, gating on C_l, k3_selective_median) zeroes the packed list's
    // length, and before a caller's halo exchange.  Only pixels this visit scanned have idx >= 0; painted ones keep the
    // refined value they were painted with.  r-bar, the K columns, C_d, C_e and the masks stay the grid winner's.
    if (!rc && form != plan::kSubgridNone)
        rc = subgrid_refine(ctx, vol, dmin_vu, dmax_vu, dmin, dmax, dim_d, s_hat, p, idx_vu, score_vu, d_depth_svu + (size_t)s_hat * n,
                            nullptr, nullptr, form == plan::kSubgridList);
    // The peaks of the pixels this visit scanned and accepted, queued here for the same two reasons; the packed list and its
    // length are read, never written, and the dense form brings lists of its own.
    if (!rc)
        rc = sweep_peaks_step(ctx, vol, dmin_vu, dmax_vu, dmin, dmax, dim_d, s_hat, p, idx_vu, pk_form);
    if (rc || !lc)
        return rc;
    ctx->sweep.lc_Ce_svu = d_Ce_svu;
    ctx->sweep.lc_dmin_vu = dmin_vu;
    ctx->sweep.lc_dmax_vu = dmax_vu;
    ctx->sweep.lc_dmin = dmin, ctx->sweep.lc_dmax = dmax, ctx->sweep.lc_dim_d = dim_d;
    ctx->sweep.lc_consts = make_scan_consts(p);
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_sweep_visit_finish(rslf_ctx* ctx, const rslf_volume* vol, int s_hat, uint8_t* d_Ce_mask_svu, float* d_Cd_svu,
                                       float* d_depth_svu, float* d_rbar_svu, const rslf_params* p) RSLF_API_TRY
{
    if (!ctx || !vol || !d_Ce_mask_svu || !d_Cd_svu || !d_depth_svu || !d_rbar_svu || !p)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (!ctx->sweep.open)
        return fail(RSLF_ERR_INVALID_ARG, "rslf_sweep_visit_finish without rslf_sweep_begin");
    if (s_hat != ctx->sweep.expect)
        return fail(RSLF_ERR_INVALID_ARG, "rslf_sweep_visit_finish(%d): the open visit is view %d", s_hat, ctx->sweep.expect);
    if (p->median_filter_size < 0 || p->median_filter_size > plan::kMedianMaxSize)
        return fail(RSLF_ERR_INVALID_ARG, "median_filter_size=%d: must be in [0, %d]", p->median_filter_size, plan::kMedianMaxSize);
    HIP_TRY(hipSetDevice(ctx->device));
    const int S = vol->S, V = vol->V, U = vol->U, C = vol->C;
    const size_t n = (size_t)V * U;
    hipStream_t st = ctx->stream;
    uint8_t* mask_svu = ctx->sweep.mask_run;
    const dim3 grid_vu((U + 255) / 256, V);
    if ((long long)S * V > (1ll << 31) - 1 || U > 65536)
        return fail(RSLF_ERR_UNSUPPORTED, "%d views x %d scanlines x %d columns: too large for one apply launch", S, V, U);
    const plan::MedianPlan mp = plan::median_plan(p->median_filter_size, C);   // window tile in LDS (k3_median.hpp)
    const plan::NormThreshold median_thr = plan::norm_threshold(p->median_filter_epsilon);
    const plan::NormThreshold prop_thr = plan::norm_threshold(p->propagation_epsilon);
    const Scratch& sc = ctx->scratch;
    float* const filtered = sc.filtered.as<float>();
    int* const winner = sc.winner.as<int>();
    uint8_t* const dirty = sc.dirty.as<uint8_t>();
    int* const remain = sc.remain.as<int>();
    int* packed_n = sc.packed_len();
    float* depth = d_depth_svu + (size_t)s_hat * n;
    float* Cd = d_Cd_svu + (size_t)s_hat * n;
    float* rbar = d_rbar_svu + (size_t)s_hat * n * C;
    uint8_t* cem = d_Ce_mask_svu + (size_t)s_hat * n;
    // core.hpp:881-892 (selective median over the edge mask) and :1088-1129 (propagation) -- the median and the
    // claims of a pixel in one launch (k34_median_claim), then the apply pass, which also lists the pixels the NEXT
    // visit scans; a visit is three launches: scan (its groups merge their records themselves), median + claims,
    // apply + compaction
    int s_next = plan::sweep_view_after(S, s_hat);
    const int s_after = s_next;
    if (ctx->force_packed == 0 || n > (size_t)INT32_MAX)
        s_next = -1;   // that scan will not take a packed list: it compacts for itself
    // Line confidence (core.hpp:1032-1081): K7 needs the FILTERED plane (:892) and, in mode 2, the claims need K7's plane.
    const int lc_mode = ctx->sweep.lc_mode;
    float* Cl = lc_mode ? ctx->sweep.lc_Cl_svu + (size_t)s_hat * n : nullptr;
    auto line_confidence = [&]() -> int {
        LineConfArgs q = {};
        q.V = V, q.S = S, q.U = U, q.s_hat = s_hat;
        q.Ce_svu = ctx->sweep.lc_Ce_svu;
        q.K_vsu = ctx->sweep.lc_K_vsu;
        q.depth_vu = filtered;
        q.mask_vu = cem;
        q.Cl_vu = Cl;
        ScanArgs a = {};
        a.vol = view_of(vol);
        a.dmin_vu = ctx->sweep.lc_dmin_vu, a.dmax_vu = ctx->sweep.lc_dmax_vu;
        a.dmin = ctx->sweep.lc_dmin, a.dmax = ctx->sweep.lc_dmax;
        a.dim_d = ctx->sweep.lc_dim_d;
        a.s_hat = s_hat;
        a.k = ctx->sweep.lc_consts;
        a.groups = 1;
        return launch_line_confidence(ctx, q, a, ctx->sweep.lc_idx_vu, C);
    };
    // core.hpp:1097-1103: C_d gates whenever use_disp_confidence_score is set, C_l in mode 2, else the edge mask
    const plan::SweepGate gate = plan::sweep_gate(p->use_disp_confidence_score != 0, lc_mode);
    const bool k7_first = plan::line_conf_before_claims(p->use_disp_confidence_score != 0, lc_mode);
    bool launched = false;
    if (k7_first) {   // the claims wait for C_l: the median alone first; k34_median_claim repeats it (tens of microseconds a plane)
#define RSLF_K3_CASE(CC, MODE)                                                                                                    \
    if (!launched && C == CC && mp.mode == MODE) {                                                                                \
        if (mp.lds_bytes > ((size_t)64 << 10))                                                                                    \
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k3_selective_median<CC, MODE>),                           \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)mp.lds_bytes));                         \
        hipLaunchKernelGGL((k3_selective_median<CC, MODE>), grid_vu, dim3(kMedianBlock), mp.lds_bytes, st, view_of(vol), depth,   \
                           filtered, cem, s_hat, mp.w, median_thr);                                                               \
        launched = true;                                                                                                          \
    }
        RSLF_MEDIAN_MODES(RSLF_K3_CASE, 1)
        RSLF_MEDIAN_MODES(RSLF_K3_CASE, 3)
#undef RSLF_K3_CASE
        if (!launched)
            return fail(RSLF_ERR_INTERNAL, "no selective-median kernel for %d channels, mode %d", C, mp.mode);
        HIP_TRY(hipGetLastError());
        if (int rc = line_confidence())
            return rc;
        launched = false;
    }
    const float* gate_vu = gate == plan::kGateDispConf ? Cd : gate == plan::kGateLineConf ? Cl : nullptr;
    const float gate_thr = gate == plan::kGateLineConf ? p->line_score_threshold : p->disp_score_threshold;
    // the gate by peak ratio: the claim kernel that takes the peaks planes; out of it, the kernel, the argument block and the
    // code of every sweep before the gate existed
    const bool gated = ctx->sweep.prop_ratio > 0.0f;
    const ClaimGate cg = {ctx->sweep.pk.idx, ctx->sweep.pk.score, ctx->sweep.pk.runner_idx, ctx->sweep.pk.runner_score,
                          (long long)s_hat * (long long)n, ctx->sweep.prop_ratio, sc.withheld.as<unsigned long long>()};
#define RSLF_K34G_CASE(CC, MODE)                                                                                                 \
    if (gated && !launched && C == CC && mp.mode == MODE) {                                                                       \
        if (mp.lds_bytes > ((size_t)64 << 10))                                                                                    \
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k34_median_claim_gated<CC, MODE>),                        \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)mp.lds_bytes));                         \
        hipLaunchKernelGGL((k34_median_claim_gated<CC, MODE>), grid_vu, dim3(256), mp.lds_bytes, st, view_of(vol), s_hat, depth,  \
                           filtered, cem, mp.w, median_thr, rbar, mask_svu, winner, dirty, p->slope_factor, prop_thr,             \
                           gate_vu, gate_thr, packed_n, ctx->claim_skip ? remain : nullptr, cg);                                  \
        launched = true;                                                                                                          \
    }
    RSLF_MEDIAN_MODES(RSLF_K34G_CASE, 1)
    RSLF_MEDIAN_MODES(RSLF_K34G_CASE, 3)
#undef RSLF_K34G_CASE
#define RSLF_K34_CASE(CC, MODE)                                                                                                  \
    if (!launched && C == CC && mp.mode == MODE) {                                                                                \
        if (mp.lds_bytes > ((size_t)64 << 10))                                                                                    \
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k34_median_claim<CC, MODE>),                              \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)mp.lds_bytes));                         \
        hipLaunchKernelGGL((k34_median_claim<CC, MODE>), grid_vu, dim3(256), mp.lds_bytes, st, view_of(vol), s_hat, depth, filtered, \
                           cem, mp.w, median_thr, rbar, mask_svu, winner, dirty, p->slope_factor, prop_thr,                       \
                           gate_vu, gate_thr, packed_n,                                                                           \
                           ctx->claim_skip ? remain : nullptr);                                                                   \
        launched = true;                                                                                                          \
    }
    RSLF_MEDIAN_MODES(RSLF_K34_CASE, 1)
    RSLF_MEDIAN_MODES(RSLF_K34_CASE, 3)
#undef RSLF_K34_CASE
    if (!launched)
        return fail(RSLF_ERR_INTERNAL, "no median + claims kernel for %d channels, mode %d", C, mp.mode);
    HIP_TRY(hipGetLastError());
    if (lc_mode != RSLF_LINE_CONF_OFF && !k7_first)
        if (int rc = line_confidence())
            return rc;
    const unsigned apply_blocks = (unsigned)((s_next >= 0 ? V : 0) + ((long long)S * V + kApplyRowsPerBlock - 1) / kApplyRowsPerBlock);
    const uint8_t* const next_mask = s_next >= 0 ? d_Ce_mask_svu + (size_t)s_next * n : nullptr;
    float* const Cl_svu = lc_mode ? ctx->sweep.lc_Cl_svu : nullptr;
    if (ctx->sweep.peaks) {   // the peaks mode's planes travel with the disparity, as C_d and C_l do: the kernel that takes them
        const rslf_peaks& pk = ctx->sweep.pk;
        const ApplyPeaks apk = {pk.idx, pk.score, pk.runner_idx, pk.runner_score};
        hipLaunchKernelGGL(k4_propagate_apply_peaks, dim3(apply_blocks), dim3(256), 0, st, S, V, U, s_hat, filtered, Cd, d_depth_svu,
                           d_Cd_svu, mask_svu, winner, dirty, s_next, next_mask, sc.list.as<int>(), sc.count.as<int>(),
                           sc.pixel_total(), packed_n, remain, sc.rowbase.as<int>(), Cl, Cl_svu, apk);
    } else {                  // out of the mode: the kernel, the argument block and the code of every sweep before the mode existed
        hipLaunchKernelGGL(k4_propagate_apply, dim3(apply_blocks), dim3(256), 0, st, S, V, U, s_hat, filtered, Cd, d_depth_svu,
                           d_Cd_svu, mask_svu, winner, dirty, s_next, next_mask, sc.list.as<int>(), sc.count.as<int>(),
                           sc.pixel_total(), packed_n, remain, sc.rowbase.as<int>(), Cl, Cl_svu);
    }
    HIP_TRY(hipGetLastError());
    ctx->sweep.listed = s_next >= 0;
    ctx->sweep.expect = s_after;
    ctx->sweep.first = false;
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_sweep_end(rslf_ctx* ctx, int ok, int dim_d, rslf_stats* stats) RSLF_API_TRY
{
    if (!ctx)
        return fail(RSLF_ERR_INVALID_ARG, "ctx is NULL");
    const bool was_open = ctx->sweep.open;
    sweep_close(ctx, ok != 0 && was_open);
    if (ok && was_open && stats) {
        HIP_TRY(hipSetDevice(ctx->device));
        return read_stats(ctx, dim_d, stats);
    }
    return RSLF_OK;
}
RSLF_API_CATCH

// What every entry below refuses before it allocates or queues anything: a bad ratio or a ratio without the peaks mode's four
// planes, a line mode that is none or lacks its plane, a subgrid that is no flag
int rslf::check_sweep_modes(const SweepModes& m)
{
    const rslf_peaks* pk = m.peaks;
    if (int rc = gate_refusal(plan::sweep_gate_entry_args(m.propagation_ratio, pk != nullptr, pk && pk->idx, pk && pk->score,
                                                          pk && pk->runner_idx, pk && pk->runner_score),
                              m.propagation_ratio, "the sweep"))
        return rc;
    if (int rc = line_conf_refusal(m.line_mode, m.Cl_svu))
        return rc;
    if (m.subgrid != 0 && m.subgrid != 1)
        return fail(RSLF_ERR_INVALID_ARG, "subgrid=%d: 0 or 1", m.subgrid);
    return RSLF_OK;
}

static bool all_planes(const SweepPlanes& o) { return o.Ce && o.Ce_mask && o.Cd && o.depth && o.rbar; }

// compute_2D_depth_epi (core.hpp:933-1133) as begin + (scan, finish) per view + end, arguments and modes already checked;
// modes.line_mode / Cl_svu: the extra argument a_line_confidence_s_v_u of the -D_USE_LINE_CONFIDENCE_SCORE build (core.hpp:345)
static int sweep_views(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu, float dmin, float dmax,
                       int dim_d, const SweepPlanes& o, const rslf_params* p, rslf_stats* stats, const SweepModes& m)
{
    int rc = check_params(p);
    if (rc)
        return rc;
    rc = rslf_sweep_begin(ctx, vol, o.Ce_mask, o.scan_mask, dim_d, 0, vol->V);
    if (rc)
        return rc;
    if (m.line_mode != RSLF_LINE_CONF_OFF)
        rc = rslf_sweep_line_confidence(ctx, vol, m.line_mode, m.Cl_svu);
    if (!rc && m.subgrid)
        rc = rslf_sweep_subgrid(ctx, vol, 1);
    if (!rc && m.peaks)
        rc = rslf_sweep_peaks(ctx, vol, m.peaks);
    if (!rc && m.propagation_ratio != 0.0f)
        rc = rslf_sweep_propagation_ratio(ctx, vol, m.propagation_ratio);
    for (int s_hat : plan::sweep_order(vol->S)) {   // core.hpp:981-990
        if (!rc)
            rc = rslf_sweep_visit_scan(ctx, vol, d_dmin_svu, d_dmax_svu, dmin, dmax, dim_d, s_hat, o.Ce, o.Ce_mask, o.Cd, o.depth, o.rbar, p);
        if (!rc)
            rc = rslf_sweep_visit_finish(ctx, vol, s_hat, o.Ce_mask, o.Cd, o.depth, o.rbar, p);
        if (rc) {
            const std::string msg = last_error_buffer();
            (void)rslf_sweep_end(ctx, 0, dim_d, nullptr);
            return fail(rc, "%s", msg.c_str());
        }
    }
    return rslf_sweep_end(ctx, 1, dim_d, stats);
}

static int depth_epi_2d(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu, float dmin,
                        float dmax, int dim_d, const SweepPlanes& d_out, const rslf_params* p, rslf_stats* stats, const SweepModes& modes)
{
    if (!ctx || !vol || !all_planes(d_out))
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (int rc = check_sweep_modes(modes))
        return rc;
    return sweep_views(ctx, vol, d_dmin_svu, d_dmax_svu, dmin, dmax, dim_d, d_out, p, stats, modes);
}

// Depth2DComputer::run (dc.hpp:748-805) on device planes, arguments and modes already checked
static int run_planes(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu, float dmin, float dmax,
                      int dim_d, const rslf_params* p, const SweepPlanes& o, rslf_stats* stats, const SweepModes& m)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n = (size_t)vol->S * vol->V * vol->U;
    hipStream_t st = ctx->stream;
    // dc.hpp:733-750 (C_e, C_d and C_l are uninitialised there; zero is the intended start)
    HIP_TRY(hipMemsetAsync(o.Ce, 0, n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(o.Cd, 0, n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(o.depth, 0, n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(o.rbar, 0, n * vol->C * sizeof(float), st));
    if (m.line_mode != RSLF_LINE_CONF_OFF)
        HIP_TRY(hipMemsetAsync(m.Cl_svu, 0, n * sizeof(float), st));   // dc.hpp:737
    if (const rslf_peaks* pk = m.peaks) {   // pixels no visit scans or paints: no index and 0, as rslf_depth_epi_peaks_host leaves unscanned ones
        if (pk->idx) HIP_TRY(hipMemsetAsync(pk->idx, 0xFF, n * sizeof(int32_t), st));
        if (pk->runner_idx) HIP_TRY(hipMemsetAsync(pk->runner_idx, 0xFF, n * sizeof(int32_t), st));
        if (pk->score) HIP_TRY(hipMemsetAsync(pk->score, 0, n * sizeof(float), st));
        if (pk->runner_score) HIP_TRY(hipMemsetAsync(pk->runner_score, 0, n * sizeof(float), st));
    }
    int rc = rslf_edge_confidence_2d(ctx, vol, p, o.Ce, o.Ce_mask);   // dc.hpp:772
    if (rc)
        return rc;
    return sweep_views(ctx, vol, d_dmin_svu, d_dmax_svu, dmin, dmax, dim_d, o, p, stats, m);   // dc.hpp:780
}

int rslf::depth2d_run(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu, float dmin, float dmax,
                      int dim_d, const rslf_params* p, const SweepPlanes& d_out, rslf_stats* stats, const SweepModes& modes)
{
    if (!ctx || !vol || !all_planes(d_out))
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (int rc = check_sweep_modes(modes))
        return rc;
    return run_planes(ctx, vol, d_dmin_svu, d_dmax_svu, dmin, dmax, dim_d, p, d_out, stats, modes);
}

// ... from a volume into host planes (each nullable; h_modes: the host's C_l plane and peak planes)
static int depth2d_run_host(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                            const SweepPlanes& h_out, rslf_stats* stats, const SweepModes& h_modes)
{
    if (!ctx || !vol)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (int rc = check_sweep_modes(h_modes))
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n = (size_t)vol->S * vol->V * vol->U;
    DevBuf Ce, Cd, depth, rbar, mask, Cl;
    HIP_TRY(Ce.alloc(n * 4));
    HIP_TRY(Cd.alloc(n * 4));
    HIP_TRY(depth.alloc(n * 4));
    HIP_TRY(rbar.alloc(n * 4 * vol->C));
    HIP_TRY(mask.alloc(n));
    if (h_modes.line_mode != RSLF_LINE_CONF_OFF)
        HIP_TRY(Cl.alloc(n * 4));
    // the peaks mode's planes: a device plane for each one the caller asks for
    const rslf_peaks* const h_pk = h_modes.peaks;
    DevBuf pk_buf[4];
    rslf_peaks d_pk = {};
    if (h_pk) {
        if (h_pk->disp)
            return fail(RSLF_ERR_INVALID_ARG, "rslf_sweep_peaks: disp must be NULL (the sub-grid mode puts that value in the depth plane)");
        const void* want[4] = {h_pk->idx, h_pk->score, h_pk->runner_idx, h_pk->runner_score};
        for (int i = 0; i < 4; i++)
            if (want[i])
                HIP_TRY(pk_buf[i].alloc(n * 4));
        d_pk.idx = pk_buf[0].as<int32_t>(), d_pk.score = pk_buf[1].as<float>();
        d_pk.runner_idx = pk_buf[2].as<int32_t>(), d_pk.runner_score = pk_buf[3].as<float>();
    }
    SweepModes d_modes = h_modes;   // the same modes on the device's planes
    d_modes.Cl_svu = Cl.as<float>();
    d_modes.peaks = h_pk ? &d_pk : nullptr;
    const SweepPlanes d_out = {Ce.as<float>(), mask.as<uint8_t>(), Cd.as<float>(), depth.as<float>(), rbar.as<float>(), nullptr};
    int rc = run_planes(ctx, vol, nullptr, nullptr, dmin, dmax, dim_d, p, d_out, stats, d_modes);
    if (rc)
        return rc;
    hipStream_t st = ctx->stream;
    if (h_pk) {
        void* to[4] = {h_pk->idx, h_pk->score, h_pk->runner_idx, h_pk->runner_score};
        for (int i = 0; i < 4; i++)
            if (to[i])
                HIP_TRY(hipMemcpyAsync(to[i], pk_buf[i].get(), n * 4, hipMemcpyDeviceToHost, st));
    }
    if (h_out.Ce) HIP_TRY(hipMemcpyAsync(h_out.Ce, Ce.get(), n * 4, hipMemcpyDeviceToHost, st));
    if (h_out.Ce_mask) HIP_TRY(hipMemcpyAsync(h_out.Ce_mask, mask.get(), n, hipMemcpyDeviceToHost, st));
    if (h_out.Cd) HIP_TRY(hipMemcpyAsync(h_out.Cd, Cd.get(), n * 4, hipMemcpyDeviceToHost, st));
    if (h_out.depth) HIP_TRY(hipMemcpyAsync(h_out.depth, depth.get(), n * 4, hipMemcpyDeviceToHost, st));
    if (h_out.rbar) HIP_TRY(hipMemcpyAsync(h_out.rbar, rbar.get(), n * 4 * vol->C, hipMemcpyDeviceToHost, st));
    if (h_modes.line_mode != RSLF_LINE_CONF_OFF) HIP_TRY(hipMemcpyAsync(h_modes.Cl_svu, Cl.get(), n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RSLF_OK;
}

// ---- the C entries: each family's wider entry adds one mode, and with that mode neutral queues exactly the narrower one's
// launches -- all of a family fill the structs and make the same call ------------------------------------------------------

extern "C" int rslf_depth_epi_2d(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu,
                                 float dmin, float dmax, int dim_d, float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu,
                                 float* d_depth_svu, float* d_rbar_svu, const rslf_params* p, uint8_t* d_scan_mask_svu,
                                 rslf_stats* stats) RSLF_API_TRY
{
    const SweepPlanes out = {d_Ce_svu, d_Ce_mask_svu, d_Cd_svu, d_depth_svu, d_rbar_svu, d_scan_mask_svu};
    return depth_epi_2d(ctx, vol, d_dmin_svu, d_dmax_svu, dmin, dmax, dim_d, out, p, stats, SweepModes());
}
RSLF_API_CATCH

// core.hpp:336-351 with a_line_confidence_s_v_u (:345)
extern "C" int rslf_depth_epi_2d_lc(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu,
                                    float dmin, float dmax, int dim_d, float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu,
                                    float* d_depth_svu, float* d_rbar_svu, const rslf_params* p, uint8_t* d_scan_mask_svu,
                                    rslf_stats* stats, int line_mode, float* d_Cl_svu) RSLF_API_TRY
{
    const SweepPlanes out = {d_Ce_svu, d_Ce_mask_svu, d_Cd_svu, d_depth_svu, d_rbar_svu, d_scan_mask_svu};
    SweepModes modes;
    modes.line_mode = line_mode, modes.Cl_svu = d_Cl_svu;
    return depth_epi_2d(ctx, vol, d_dmin_svu, d_dmax_svu, dmin, dmax, dim_d, out, p, stats, modes);
}
RSLF_API_CATCH

// ... and the sub-grid mode
extern "C" int rslf_depth_epi_2d_sub(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu,
                                     float dmin, float dmax, int dim_d, float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu,
                                     float* d_depth_svu, float* d_rbar_svu, const rslf_params* p, uint8_t* d_scan_mask_svu,
                                     rslf_stats* stats, int line_mode, float* d_Cl_svu, int subgrid) RSLF_API_TRY
{
    const SweepPlanes out = {d_Ce_svu, d_Ce_mask_svu, d_Cd_svu, d_depth_svu, d_rbar_svu, d_scan_mask_svu};
    SweepModes modes;
    modes.line_mode = line_mode, modes.Cl_svu = d_Cl_svu, modes.subgrid = subgrid;
    return depth_epi_2d(ctx, vol, d_dmin_svu, d_dmax_svu, dmin, dmax, dim_d, out, p, stats, modes);
}
RSLF_API_CATCH

// ... and the peaks mode (rslf_sweep_peaks)
extern "C" int rslf_depth_epi_2d_pk(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu,
                                    float dmin, float dmax, int dim_d, float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu,
                                    float* d_depth_svu, float* d_rbar_svu, const rslf_params* p, uint8_t* d_scan_mask_svu,
                                    rslf_stats* stats, int line_mode, float* d_Cl_svu, int subgrid, const rslf_peaks* d_pk_svu) RSLF_API_TRY
{
    const SweepPlanes out = {d_Ce_svu, d_Ce_mask_svu, d_Cd_svu, d_depth_svu, d_rbar_svu, d_scan_mask_svu};
    SweepModes modes;
    modes.line_mode = line_mode, modes.Cl_svu = d_Cl_svu, modes.subgrid = subgrid, modes.peaks = d_pk_svu;
    return depth_epi_2d(ctx, vol, d_dmin_svu, d_dmax_svu, dmin, dmax, dim_d, out, p, stats, modes);
}
RSLF_API_CATCH

// ... and the gate by peak ratio (rslf_sweep_propagation_ratio)
extern "C" int rslf_depth_epi_2d_pr(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_svu, const float* d_dmax_svu,
                                    float dmin, float dmax, int dim_d, float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu,
                                    float* d_depth_svu, float* d_rbar_svu, const rslf_params* p, uint8_t* d_scan_mask_svu,
                                    rslf_stats* stats, int line_mode, float* d_Cl_svu, int subgrid, const rslf_peaks* d_pk_svu,
                                    float propagation_ratio) RSLF_API_TRY
{
    const SweepPlanes out = {d_Ce_svu, d_Ce_mask_svu, d_Cd_svu, d_depth_svu, d_rbar_svu, d_scan_mask_svu};
    SweepModes modes;
    modes.line_mode = line_mode, modes.Cl_svu = d_Cl_svu, modes.subgrid = subgrid, modes.peaks = d_pk_svu;
    modes.propagation_ratio = propagation_ratio;
    return depth_epi_2d(ctx, vol, d_dmin_svu, d_dmax_svu, dmin, dmax, dim_d, out, p, stats, modes);
}
RSLF_API_CATCH

extern "C" int rslf_depth2d_run(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                                float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu, float* d_depth_svu, float* d_rbar_svu,
                                uint8_t* d_scan_mask_svu, rslf_stats* stats) RSLF_API_TRY
{
    const SweepPlanes out = {d_Ce_svu, d_Ce_mask_svu, d_Cd_svu, d_depth_svu, d_rbar_svu, d_scan_mask_svu};
    return depth2d_run(ctx, vol, nullptr, nullptr, dmin, dmax, dim_d, p, out, stats, SweepModes());
}
RSLF_API_CATCH

// dc.hpp:748-805 with the line-confidence planes of dc.hpp:721-738, :791-792
extern "C" int rslf_depth2d_run_lc(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                                   float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu, float* d_depth_svu, float* d_rbar_svu,
                                   uint8_t* d_scan_mask_svu, rslf_stats* stats, int line_mode, float* d_Cl_svu) RSLF_API_TRY
{
    const SweepPlanes out = {d_Ce_svu, d_Ce_mask_svu, d_Cd_svu, d_depth_svu, d_rbar_svu, d_scan_mask_svu};
    SweepModes modes;
    modes.line_mode = line_mode, modes.Cl_svu = d_Cl_svu;
    return depth2d_run(ctx, vol, nullptr, nullptr, dmin, dmax, dim_d, p, out, stats, modes);
}
RSLF_API_CATCH

// ... and the sub-grid mode of every visit (rslf_sweep_subgrid)
extern "C" int rslf_depth2d_run_sub(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                                    float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu, float* d_depth_svu, float* d_rbar_svu,
                                    uint8_t* d_scan_mask_svu, rslf_stats* stats, int line_mode, float* d_Cl_svu, int subgrid) RSLF_API_TRY
{
    const SweepPlanes out = {d_Ce_svu, d_Ce_mask_svu, d_Cd_svu, d_depth_svu, d_rbar_svu, d_scan_mask_svu};
    SweepModes modes;
    modes.line_mode = line_mode, modes.Cl_svu = d_Cl_svu, modes.subgrid = subgrid;
    return depth2d_run(ctx, vol, nullptr, nullptr, dmin, dmax, dim_d, p, out, stats, modes);
}
RSLF_API_CATCH

// ... and the peaks mode of every visit (rslf_sweep_peaks)
extern "C" int rslf_depth2d_run_pk(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                                   float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu, float* d_depth_svu, float* d_rbar_svu,
                                   uint8_t* d_scan_mask_svu, rslf_stats* stats, int line_mode, float* d_Cl_svu, int subgrid,
                                   const rslf_peaks* d_pk_svu) RSLF_API_TRY
{
    const SweepPlanes out = {d_Ce_svu, d_Ce_mask_svu, d_Cd_svu, d_depth_svu, d_rbar_svu, d_scan_mask_svu};
    SweepModes modes;
    modes.line_mode = line_mode, modes.Cl_svu = d_Cl_svu, modes.subgrid = subgrid, modes.peaks = d_pk_svu;
    return depth2d_run(ctx, vol, nullptr, nullptr, dmin, dmax, dim_d, p, out, stats, modes);
}
RSLF_API_CATCH

// ... and the gate by peak ratio
extern "C" int rslf_depth2d_run_pr(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                                   float* d_Ce_svu, uint8_t* d_Ce_mask_svu, float* d_Cd_svu, float* d_depth_svu, float* d_rbar_svu,
                                   uint8_t* d_scan_mask_svu, rslf_stats* stats, int line_mode, float* d_Cl_svu, int subgrid,
                                   const rslf_peaks* d_pk_svu, float propagation_ratio) RSLF_API_TRY
{
    const SweepPlanes out = {d_Ce_svu, d_Ce_mask_svu, d_Cd_svu, d_depth_svu, d_rbar_svu, d_scan_mask_svu};
    SweepModes modes;
    modes.line_mode = line_mode, modes.Cl_svu = d_Cl_svu, modes.subgrid = subgrid, modes.peaks = d_pk_svu;
    modes.propagation_ratio = propagation_ratio;
    return depth2d_run(ctx, vol, nullptr, nullptr, dmin, dmax, dim_d, p, out, stats, modes);
}
RSLF_API_CATCH

extern "C" int rslf_depth2d_run_host(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                                     float* h_Ce_svu, uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu,
                                     float* h_rbar_svu, rslf_stats* stats) RSLF_API_TRY
{
    const SweepPlanes out = {h_Ce_svu, h_Ce_mask_svu, h_Cd_svu, h_depth_svu, h_rbar_svu, nullptr};
    return depth2d_run_host(ctx, vol, dmin, dmax, dim_d, p, out, stats, SweepModes());
}
RSLF_API_CATCH

extern "C" int rslf_depth2d_run_host_lc(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                                        float* h_Ce_svu, uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu,
                                        float* h_rbar_svu, rslf_stats* stats, int line_mode, float* h_Cl_svu) RSLF_API_TRY
{
    const SweepPlanes out = {h_Ce_svu, h_Ce_mask_svu, h_Cd_svu, h_depth_svu, h_rbar_svu, nullptr};
    SweepModes modes;
    modes.line_mode = line_mode, modes.Cl_svu = h_Cl_svu;
    return depth2d_run_host(ctx, vol, dmin, dmax, dim_d, p, out, stats, modes);
}
RSLF_API_CATCH

extern "C" int rslf_depth2d_run_host_sub(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                                         float* h_Ce_svu, uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu,
                                         float* h_rbar_svu, rslf_stats* stats, int line_mode, float* h_Cl_svu, int subgrid) RSLF_API_TRY
{
    const SweepPlanes out = {h_Ce_svu, h_Ce_mask_svu, h_Cd_svu, h_depth_svu, h_rbar_svu, nullptr};
    SweepModes modes;
    modes.line_mode = line_mode, modes.Cl_svu = h_Cl_svu, modes.subgrid = subgrid;
    return depth2d_run_host(ctx, vol, dmin, dmax, dim_d, p, out, stats, modes);
}
RSLF_API_CATCH

extern "C" int rslf_depth2d_run_host_pk(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                                        float* h_Ce_svu, uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu,
                                        float* h_rbar_svu, rslf_stats* stats, int line_mode, float* h_Cl_svu, int subgrid,
                                        const rslf_peaks* h_pk_svu) RSLF_API_TRY
{
    const SweepPlanes out = {h_Ce_svu, h_Ce_mask_svu, h_Cd_svu, h_depth_svu, h_rbar_svu, nullptr};
    SweepModes modes;
    modes.line_mode = line_mode, modes.Cl_svu = h_Cl_svu, modes.subgrid = subgrid, modes.peaks = h_pk_svu;
    return depth2d_run_host(ctx, vol, dmin, dmax, dim_d, p, out, stats, modes);
}
RSLF_API_CATCH

extern "C" int rslf_depth2d_run_host_pr(rslf_ctx* ctx, const rslf_volume* vol, float dmin, float dmax, int dim_d, const rslf_params* p,
                                        float* h_Ce_svu, uint8_t* h_Ce_mask_svu, float* h_Cd_svu, float* h_depth_svu,
                                        float* h_rbar_svu, rslf_stats* stats, int line_mode, float* h_Cl_svu, int subgrid,
                                        const rslf_peaks* h_pk_svu, float propagation_ratio) RSLF_API_TRY
{
    const SweepPlanes out = {h_Ce_svu, h_Ce_mask_svu, h_Cd_svu, h_depth_svu, h_rbar_svu, nullptr};
    SweepModes modes;
    modes.line_mode = line_mode, modes.Cl_svu = h_Cl_svu, modes.subgrid = subgrid, modes.peaks = h_pk_svu;
    modes.propagation_ratio = propagation_ratio;
    return depth2d_run_host(ctx, vol, dmin, dmax, dim_d, p, out, stats, modes);
}
RSLF_API_CATCH
