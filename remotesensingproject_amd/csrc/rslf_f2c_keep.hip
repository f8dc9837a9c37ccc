// A finished fine-to-coarse run kept on the device (include/rslf_hip.h, "fine-to-coarse kept on the device"): rslf_f2c_run
// owns what the level loop of rslf_f2c.hip allocates (F2cKept), hands planes out by copy, and renders the three coloured
// getters of rslf_fine_to_coarse.hpp:325-519 from them with the renderers of rslf_render.hip.  No kernels of its own.
#include "rslf_internal.hpp"
#include "rslf_plan_f2c_consistency.hpp"
#include "rslf_plan_f2c_peaks.hpp"
#include "rslf_plan_sweep_gate.hpp"

using namespace rslf;

namespace {

bool is_peak_plane(int which) { return which >= RSLF_F2C_PLANE_PK_IDX && which <= RSLF_F2C_PLANE_FUSED_LEVEL; }
bool is_gate_plane(int which) { return which == RSLF_F2C_PLANE_CS_AGREE || which == RSLF_F2C_PLANE_CS_SEEN; }
bool is_fused_plane(int which)
{
    return which == RSLF_F2C_PLANE_FUSED_MAP || which == RSLF_F2C_PLANE_FUSED_VALID ||
           (which >= RSLF_F2C_PLANE_FUSED_PK_IDX && which <= RSLF_F2C_PLANE_FUSED_LEVEL);
}

// A plane of the run: where it lies and how many bytes it has; NULL if it is not held.
const void* plane_of(const rslf_f2c_run* run, int level, int which, size_t* bytes)
{
    const F2cKeptLevel& kl = run->kept.levels[(size_t)level];
    const size_t n = (size_t)run->S * kl.V * kl.U;
    *bytes = n * sizeof(float);
    switch (which) {
    case RSLF_F2C_PLANE_DEPTH:
        return kl.depth.get();
    case RSLF_F2C_PLANE_VALID:
        *bytes = n;
        return kl.valid.get();
    case RSLF_F2C_PLANE_CE:
        return kl.Ce.get();
    case RSLF_F2C_PLANE_CD:
        return kl.Cd.get();
    case RSLF_F2C_PLANE_CL:
        return kl.Cl.get();
    case RSLF_F2C_PLANE_FUSED_MAP:
        return run->kept.fused_map.get();
    case RSLF_F2C_PLANE_FUSED_VALID:
        *bytes = n;
        return run->kept.fused_valid.get();
    case RSLF_F2C_PLANE_PK_IDX:
        return kl.pk_idx.get();
    case RSLF_F2C_PLANE_PK_SCORE:
        return kl.pk_score.get();
    case RSLF_F2C_PLANE_PK_RUNNER_IDX:
        return kl.pk_runner_idx.get();
    case RSLF_F2C_PLANE_PK_RUNNER_SCORE:
        return kl.pk_runner_score.get();
    case RSLF_F2C_PLANE_FUSED_PK_IDX:
        return run->kept.fused_pk_idx.get();
    case RSLF_F2C_PLANE_FUSED_PK_SCORE:
        return run->kept.fused_pk_score.get();
    case RSLF_F2C_PLANE_FUSED_PK_RUNNER_IDX:
        return run->kept.fused_pk_runner_idx.get();
    case RSLF_F2C_PLANE_FUSED_PK_RUNNER_SCORE:
        return run->kept.fused_pk_runner_score.get();
    case RSLF_F2C_PLANE_FUSED_LEVEL:
        *bytes = n;
        return run->kept.fused_level.get();
    case RSLF_F2C_PLANE_CS_AGREE:
        return kl.cs_agree.get();
    case RSLF_F2C_PLANE_CS_SEEN:
        return kl.cs_seen.get();
    }
    return nullptr;
}

// The two wordings of "the run has no such level"
int check_level_outside(const rslf_f2c_run* run, int level)
{
    if (level < 0 || level >= (int)run->kept.levels.size())
        return fail(RSLF_ERR_INVALID_ARG, "level=%d outside [0,%d)", level, (int)run->kept.levels.size());
    return RSLF_OK;
}
int check_level_of(const rslf_f2c_run* run, int level)
{
    if (level < 0 || level >= (int)run->kept.levels.size())
        return fail(RSLF_ERR_INVALID_ARG, "level %d of %d", level, (int)run->kept.levels.size());
    return RSLF_OK;
}

int check_render_args(const rslf_f2c_run* run, const rslf_ctx* ctx, const void* lut_bgr, const void* out)
{
    if (!run || !ctx || !lut_bgr || !out)
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    if (ctx->device != run->device)
        return fail(RSLF_ERR_INVALID_ARG, "the run lives on device %d, the context on device %d", run->device, ctx->device);
    return RSLF_OK;
}

// The volume of the getters' shadow cut (f2c.hpp:360-372, :466-481) as the renderers take it: a non-owning copy of the
// kept volume's description that names the rendering context (the context the run was made on may be gone).
int shadow_volume(const rslf_f2c_run* run, rslf_ctx* ctx, int level, rslf_volume* view, const rslf_volume** out)
{
    *out = nullptr;
    if (!run->params.cut_shadows)
        return RSLF_OK;
    const rslf_volume* vol = run->kept.levels[(size_t)level].vol.get();
    if (!vol)
        return fail(RSLF_ERR_INVALID_ARG, "the run was made with cut_shadows but without keep_volumes: the shadow cut reads the "
                                          "level's volume, which was not kept");
    *view = *vol;
    view->ctx = ctx;
    *out = view;
    return RSLF_OK;
}

int fit_mode(int saturate) { return saturate ? RSLF_FIT_QUANTILE : RSLF_FIT_MEANSTD; }   // ImageConverter_uchar::fit(img, saturate)

// One picture of a getter: where it goes in the caller's memory and how large it is.
struct Picture {
    uint8_t* dst;
    size_t bytes;
};

// The pictures are rendered into the caller's device memory, or -- host form -- into the context's staging buffer and copied
// out from there; `pics` holds the caller's pointers, `targets` gets the device pointers to render into.
int stage_pictures(rslf_ctx* ctx, bool host, const std::vector<Picture>& pics, std::vector<uint8_t*>* targets)
{
    targets->resize(pics.size());
    size_t total = 0;
    for (const Picture& p : pics)
        total += p.bytes;
    void* stage = nullptr;
    if (host) {
        int rc = helper_scratch(ctx, kSharedStageOut, total, &stage);
        if (rc)
            return rc;
    }
    size_t o = 0;
    for (size_t i = 0; i < pics.size(); i++) {
        (*targets)[i] = host ? (uint8_t*)stage + o : pics[i].dst;
        o += pics[i].bytes;
    }
    return RSLF_OK;
}

int deliver_pictures(rslf_ctx* ctx, bool host, const std::vector<Picture>& pics, const std::vector<uint8_t*>& targets)
{
    if (!host)
        return RSLF_OK;   // enqueued, not awaited
    for (size_t i = 0; i < pics.size(); i++)
        HIP_TRY(hipMemcpyAsync(pics[i].dst, targets[i], pics[i].bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RSLF_OK;
}

// get_coloured_depth_maps, rslf_fine_to_coarse.hpp:325-378
int render_depth_maps(const rslf_f2c_run* run, rslf_ctx* ctx, int saturate, const uint8_t* lut_bgr, uint8_t* out, bool host)
{
    int rc = check_render_args(run, ctx, lut_bgr, out);
    if (rc)
        return rc;
    const F2cKeptLevel& l0 = run->kept.levels[0];
    const int S = run->S, V = l0.V, U = l0.U;
    int mid = 0;
    rc = rslf_render_centre_index(S, &mid);   // :344
    if (rc)
        return rc;
    rslf_volume view;
    const rslf_volume* vol = nullptr;
    rc = shadow_volume(run, ctx, 0, &view, &vol);
    if (rc)
        return rc;
    const std::vector<Picture> pics = {{out, (size_t)S * V * U * 3}};
    std::vector<uint8_t*> target;
    rc = stage_pictures(ctx, host, pics, &target);
    if (rc)
        return rc;
    const float* map = run->kept.fused_map.as<const float>();
    double lo = 0.0, hi = 0.0;
    rc = rslf_render_fit(ctx, map + (size_t)mid * V * U, V, U, (size_t)U, nullptr, fit_mode(saturate), &lo, &hi);
    if (!rc)
        rc = rslf_render_planes(ctx, map, S, (size_t)V * U, V, U, (size_t)U, lo, hi, RSLF_RENDER_AFFINE, lut_bgr,
                                run->kept.fused_valid.as<const uint8_t>(), RSLF_MASK_BLACK, vol, RSLF_SLICE_VIEW, 0,
                                run->params.shadow_level, target[0]);
    if (rc)
        return rc;
    return deliver_pictures(ctx, host, pics, target);
}

// get_coloured_depth_pyr, :491-519
int render_depth_pyr(const rslf_f2c_run* run, rslf_ctx* ctx, int s, int saturate, const uint8_t* lut_bgr, uint8_t* const* out, bool host)
{
    int rc = check_render_args(run, ctx, lut_bgr, out);
    if (rc)
        return rc;
    const int S = run->S, P = (int)run->kept.levels.size();
    if (s == -1) {
        rc = rslf_render_centre_index(S, &s);   // :497
        if (rc)
            return rc;
    }
    if (s < 0 || s >= S)
        return fail(RSLF_ERR_INVALID_ARG, "view %d of %d", s, S);
    std::vector<Picture> pics((size_t)P);
    for (int l = 0; l < P; l++) {
        if (!out[l])
            return fail(RSLF_ERR_INVALID_ARG, "out[%d] is NULL", l);
        pics[(size_t)l] = {out[l], (size_t)run->kept.levels[(size_t)l].V * run->kept.levels[(size_t)l].U * 3};
    }
    std::vector<uint8_t*> target;
    rc = stage_pictures(ctx, host, pics, &target);
    if (rc)
        return rc;
    double lo = 0.0, hi = 0.0;
    for (int l = 0; l < P; l++) {
        const F2cKeptLevel& kl = run->kept.levels[(size_t)l];
        const size_t o = (size_t)s * kl.V * kl.U;
        const float* plane = kl.depth.as<const float>() + o;
        if (l == 0) {   // the converter is fitted on level 0's plane before any masking
            rc = rslf_render_fit(ctx, plane, kl.V, kl.U, (size_t)kl.U, nullptr, fit_mode(saturate), &lo, &hi);
            if (rc)
                return rc;
        }
        rc = rslf_render_planes(ctx, plane, 1, 0, kl.V, kl.U, (size_t)kl.U, lo, hi, RSLF_RENDER_AFFINE, lut_bgr,
                                kl.valid.as<const uint8_t>() + o, RSLF_MASK_BLACK, nullptr, RSLF_SLICE_VIEW, 0, 0.0f, target[(size_t)l]);
        if (rc)
            return rc;
    }
    return deliver_pictures(ctx, host, pics, target);
}

// get_coloured_epi_pyr, :432-488
int render_epi_pyr(const rslf_f2c_run* run, rslf_ctx* ctx, int v, int saturate, const uint8_t* lut_bgr, uint8_t* const* out, bool host)
{
    int rc = check_render_args(run, ctx, lut_bgr, out);
    if (rc)
        return rc;
    const int S = run->S, P = (int)run->kept.levels.size(), V0 = run->kept.levels[0].V;
    if (v == -1) {
        rc = rslf_render_centre_index(V0, &v);
        if (rc)
            return rc;
    }
    std::vector<int> row((size_t)P);
    std::vector<Picture> pics((size_t)P);
    std::vector<rslf_volume> views((size_t)P);
    std::vector<const rslf_volume*> vols((size_t)P, nullptr);
    for (int l = 0; l < P; l++) {   // every refusal before anything is queued
        const F2cKeptLevel& kl = run->kept.levels[(size_t)l];
        rc = rslf_render_scaled_row(v, kl.V, V0, &row[(size_t)l]);   // :451
        if (!rc)
            rc = shadow_volume(run, ctx, l, &views[(size_t)l], &vols[(size_t)l]);
        if (rc)
            return rc;
        if (!out[l])
            return fail(RSLF_ERR_INVALID_ARG, "out[%d] is NULL", l);
        pics[(size_t)l] = {out[l], (size_t)S * kl.U * 3};
    }
    std::vector<uint8_t*> target;
    rc = stage_pictures(ctx, host, pics, &target);
    if (rc)
        return rc;
    double lo = 0.0, hi = 0.0;
    for (int l = 0; l < P; l++) {
        const F2cKeptLevel& kl = run->kept.levels[(size_t)l];
        const size_t o = (size_t)row[(size_t)l] * kl.U, stride = (size_t)kl.V * kl.U;   // row `row` of every view: an S x U_l plane
        const float* plane = kl.depth.as<const float>() + o;
        const uint8_t* valid = kl.valid.as<const uint8_t>() + o;
        if (l == 0) {   // fitted on level 0, its invalid pixels counting as 0 (:458-459)
            rc = rslf_render_fit(ctx, plane, S, kl.U, stride, valid, fit_mode(saturate), &lo, &hi);
            if (rc)
                return rc;
        }
        rc = rslf_render_planes(ctx, plane, 1, 0, S, kl.U, stride, lo, hi, RSLF_RENDER_AFFINE, lut_bgr, valid, RSLF_MASK_ZERO_VALUE,
                                vols[(size_t)l], RSLF_SLICE_EPI, row[(size_t)l], run->params.shadow_level, target[(size_t)l]);
        if (rc)
            return rc;
    }
    return deliver_pictures(ctx, host, pics, target);
}

}  // namespace

// A pyramid run and kept: req.elem comes from `elem` here, everything else of req and o as the entry filled it.
static int f2c_run_host(rslf_ctx* ctx, int elem, F2cRequest req, const F2cOptions& o, rslf_f2c_run** run, rslf_stats* stats)
{
    if (!run)
        return fail(RSLF_ERR_INVALID_ARG, "run is NULL");
    *run = nullptr;
    if (!ctx || !req.h_epis || !req.p)
        return fail(RSLF_ERR_INVALID_ARG, "bad arguments");
    switch (plan::f2c_peaks_args(o.peaks, o.uniqueness, req.dim_d)) {
    case plan::kF2cPeaksOk:
        break;
    case plan::kF2cPeaksBadFlag:
        return fail(RSLF_ERR_INVALID_ARG, "peaks=%d: 0 or 1", o.peaks);
    case plan::kF2cPeaksBadRatio:
        return fail(RSLF_ERR_INVALID_ARG, "uniqueness_ratio=%g: 0 (off) or a ratio in (0, 1]", (double)o.uniqueness);
    case plan::kF2cPeaksRatioAlone:
        return fail(RSLF_ERR_INVALID_ARG, "uniqueness_ratio=%g reads the peak planes: it needs peaks = 1", (double)o.uniqueness);
    case plan::kF2cPeaksBadDimD:
        return fail(RSLF_ERR_INVALID_ARG, "dim_d=%d: the peaks take at most %d hypotheses", req.dim_d, plan::kPeakMaxDimD);
    }
    // the sweeps' gate by peak ratio: independent of the uniqueness ratio; it reads the levels' peak planes
    if (!plan::sweep_gate_ratio_ok(o.propagation_ratio))
        return fail(RSLF_ERR_INVALID_ARG, "propagation_ratio=%g: 0 (off) or a ratio in (0, 1]", (double)o.propagation_ratio);
    if (o.propagation_ratio != 0.0f && !o.peaks)
        return fail(RSLF_ERR_INVALID_ARG, "propagation_ratio=%g reads the peak planes: it needs peaks = 1", (double)o.propagation_ratio);
    // the validity by cross-view consistency: independent of the peaks; 0 is off, and then tol and radius are not looked at
    switch (plan::f2c_consistency_args(o.cs_tol, o.cs_min_agree)) {
    case plan::kF2cConsistencyOk:
        break;
    case plan::kF2cConsistencyBadMinAgree:
        return fail(RSLF_ERR_INVALID_ARG, "consistency_min_agree=%d: 0 (off) or a count of agreeing views >= 1", o.cs_min_agree);
    case plan::kF2cConsistencyBadTol:
        return fail(RSLF_ERR_INVALID_ARG, "consistency_tol=%g: a finite tolerance >= 0", (double)o.cs_tol);
    }
    if (int rc = check_level_dilation(o))
        return rc;
    if (int rc = check_equalize(o, req.V, req.S, req.U, req.C))
        return rc;
    // (the level's sweeps would end a sweep the caller left open; the entries without the gate do what they always did)
    if (o.cs_min_agree > 0 && ctx->sweep.open)
        return fail(RSLF_ERR_INVALID_ARG, "consistency_min_agree: a sweep is open on this context");
    int rc = elem_of(elem, &req.elem);
    if (rc)
        return rc;
    if ((int)plan::f2c_pyramid(req.V, req.U, req.max_pyr_depth).size() > RSLF_F2C_MAX_LEVELS)
        return fail(RSLF_ERR_UNSUPPORTED, "a pyramid deeper than %d levels", RSLF_F2C_MAX_LEVELS);
    // (the finest level has the largest grid; a shape that is none is refused by the loop)
    if (o.cs_min_agree > 0 && req.S >= 1 && req.V >= 1 && req.U >= 1 && !plan::consistency_grid(req.S, req.V, req.U))
        return fail(RSLF_ERR_UNSUPPORTED, "consistency_min_agree: S=%d V=%d U=%d exceed the grid limit of one gate launch (or U > %d)", req.S,
                    req.V, req.U, plan::kConsistencyMaxU);
    std::unique_ptr<rslf_f2c_run> r(new rslf_f2c_run());   // whatever path leaves this function, a run not handed out is freed
    r->device = ctx->device;
    r->S = req.S;
    r->C = o.derivative_weight > 0.0f ? 3 : req.C;   // (with the derivative channels the run is a three-channel run; the loop refuses C != 1)
    r->elem = elem;
    r->params = *req.p;
    r->options = o;
    if (o.cs_min_agree == 0)   // off: tol and radius were not looked at, and the run reports none
        r->options.cs_tol = 0.0f, r->options.cs_radius = 0;
    rc = fine_to_coarse_one_context(ctx, req, r->options, F2cHostOut(), stats, &r->kept);
    if (rc)
        return rc;
    *run = r.release();
    return RSLF_OK;
}

// The kept-run entries: the same call, the request in the order of their arguments; what an entry lacks stays off.

extern "C" int rslf_f2c_run_host(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C, size_t row_stride_bytes,
                                 float d_min, float d_max, int dim_d, float epi_scale_factor, const rslf_params* p, int max_pyr_depth,
                                 int accept_all_last_scale, int line_mode, int validity_rule, int keep_volumes, rslf_f2c_run** run,
                                 rslf_stats* stats) RSLF_API_TRY
{
    const F2cRequest req = {Elem::F32, h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p, max_pyr_depth,
                            accept_all_last_scale};
    F2cOptions o;
    o.line_mode = line_mode, o.validity_rule = validity_rule, o.keep_volumes = keep_volumes != 0;
    return f2c_run_host(ctx, elem, req, o, run, stats);
}
RSLF_API_CATCH

// ... every level's sweep in the sub-grid mode (rslf_sweep_subgrid)
extern "C" int rslf_f2c_run_host_sub(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C,
                                     size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                     const rslf_params* p, int max_pyr_depth, int accept_all_last_scale, int line_mode,
                                     int validity_rule, int keep_volumes, rslf_f2c_run** run, rslf_stats* stats, int subgrid) RSLF_API_TRY
{
    const F2cRequest req = {Elem::F32, h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p, max_pyr_depth,
                            accept_all_last_scale};
    F2cOptions o;
    o.line_mode = line_mode, o.validity_rule = validity_rule, o.keep_volumes = keep_volumes != 0, o.subgrid = subgrid;
    return f2c_run_host(ctx, elem, req, o, run, stats);
}
RSLF_API_CATCH

// ... and with peaks = 1 every level's sweep in the peaks mode as well (rslf_sweep_peaks), the four planes of every level and
// the fused peaks kept; uniqueness_ratio > 0: validity by uniqueness
extern "C" int rslf_f2c_run_host_pk(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C,
                                    size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                    const rslf_params* p, int max_pyr_depth, int accept_all_last_scale, int line_mode,
                                    int validity_rule, int keep_volumes, rslf_f2c_run** run, rslf_stats* stats, int subgrid, int peaks,
                                    float uniqueness_ratio) RSLF_API_TRY
{
    const F2cRequest req = {Elem::F32, h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p, max_pyr_depth,
                            accept_all_last_scale};
    F2cOptions o;
    o.line_mode = line_mode, o.validity_rule = validity_rule, o.keep_volumes = keep_volumes != 0, o.subgrid = subgrid;
    o.peaks = peaks, o.uniqueness = uniqueness_ratio;
    return f2c_run_host(ctx, elem, req, o, run, stats);
}
RSLF_API_CATCH

// ... and with propagation_ratio > 0 every level's sweep gated by it (rslf_sweep_propagation_ratio)
extern "C" int rslf_f2c_run_host_pr(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C,
                                    size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                    const rslf_params* p, int max_pyr_depth, int accept_all_last_scale, int line_mode,
                                    int validity_rule, int keep_volumes, rslf_f2c_run** run, rslf_stats* stats, int subgrid, int peaks,
                                    float uniqueness_ratio, float propagation_ratio) RSLF_API_TRY
{
    const F2cRequest req = {Elem::F32, h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p, max_pyr_depth,
                            accept_all_last_scale};
    F2cOptions o;
    o.line_mode = line_mode, o.validity_rule = validity_rule, o.keep_volumes = keep_volumes != 0, o.subgrid = subgrid;
    o.peaks = peaks, o.uniqueness = uniqueness_ratio, o.propagation_ratio = propagation_ratio;
    return f2c_run_host(ctx, elem, req, o, run, stats);
}
RSLF_API_CATCH

// ... and with consistency_min_agree > 0 every level's validity gated by the other views (k13_f2c_consistency_gate)
extern "C" int rslf_f2c_run_host_cs(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C,
                                    size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                    const rslf_params* p, int max_pyr_depth, int accept_all_last_scale, int line_mode,
                                    int validity_rule, int keep_volumes, rslf_f2c_run** run, rslf_stats* stats, int subgrid, int peaks,
                                    float uniqueness_ratio, float propagation_ratio, float consistency_tol, int consistency_radius,
                                    int consistency_min_agree) RSLF_API_TRY
{
    const F2cRequest req = {Elem::F32, h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p, max_pyr_depth,
                            accept_all_last_scale};
    F2cOptions o;
    o.line_mode = line_mode, o.validity_rule = validity_rule, o.keep_volumes = keep_volumes != 0, o.subgrid = subgrid;
    o.peaks = peaks, o.uniqueness = uniqueness_ratio, o.propagation_ratio = propagation_ratio;
    o.cs_tol = consistency_tol, o.cs_radius = consistency_radius, o.cs_min_agree = consistency_min_agree;
    return f2c_run_host(ctx, elem, req, o, run, stats);
}
RSLF_API_CATCH

// ... and with derivative_weight > 0 a one-channel field goes down the pyramid as (x, |dx/du|, |dx/dv|) (K17): the run is a
// three-channel run
extern "C" int rslf_f2c_run_host_dv(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C,
                                    size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                    const rslf_params* p, int max_pyr_depth, int accept_all_last_scale, int line_mode,
                                    int validity_rule, int keep_volumes, rslf_f2c_run** run, rslf_stats* stats, int subgrid, int peaks,
                                    float uniqueness_ratio, float propagation_ratio, float consistency_tol, int consistency_radius,
                                    int consistency_min_agree, float derivative_weight) RSLF_API_TRY
{
    const F2cRequest req = {Elem::F32, h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p, max_pyr_depth,
                            accept_all_last_scale};
    F2cOptions o;
    o.line_mode = line_mode, o.validity_rule = validity_rule, o.keep_volumes = keep_volumes != 0, o.subgrid = subgrid;
    o.peaks = peaks, o.uniqueness = uniqueness_ratio, o.propagation_ratio = propagation_ratio;
    o.cs_tol = consistency_tol, o.cs_radius = consistency_radius, o.cs_min_agree = consistency_min_agree;
    o.derivative_weight = derivative_weight;
    return f2c_run_host(ctx, elem, req, o, run, stats);
}
RSLF_API_CATCH

// ... and with level_dilation > 1 every level's sweep in the frame dilated along u, its planes back on the level's grid (K18)
extern "C" int rslf_f2c_run_host_dl(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C,
                                    size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                    const rslf_params* p, int max_pyr_depth, int accept_all_last_scale, int line_mode,
                                    int validity_rule, int keep_volumes, rslf_f2c_run** run, rslf_stats* stats, int subgrid, int peaks,
                                    float uniqueness_ratio, float propagation_ratio, float consistency_tol, int consistency_radius,
                                    int consistency_min_agree, float derivative_weight, int level_dilation, int dilation_kind) RSLF_API_TRY
{
    const F2cRequest req = {Elem::F32, h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p, max_pyr_depth,
                            accept_all_last_scale};
    F2cOptions o;
    o.line_mode = line_mode, o.validity_rule = validity_rule, o.keep_volumes = keep_volumes != 0, o.subgrid = subgrid;
    o.peaks = peaks, o.uniqueness = uniqueness_ratio, o.propagation_ratio = propagation_ratio;
    o.cs_tol = consistency_tol, o.cs_radius = consistency_radius, o.cs_min_agree = consistency_min_agree;
    o.derivative_weight = derivative_weight;
    o.level_dilation = level_dilation, o.dilation_kind = dilation_kind;
    return f2c_run_host(ctx, elem, req, o, run, stats);
}
RSLF_API_CATCH

// ... and with equalize_mode != 0 the finest level's upload equalised per view before anything reads it (K19)
extern "C" int rslf_f2c_run_host_eq(rslf_ctx* ctx, const void* const* h_epis, int elem, int V, int S, int U, int C,
                                    size_t row_stride_bytes, float d_min, float d_max, int dim_d, float epi_scale_factor,
                                    const rslf_params* p, int max_pyr_depth, int accept_all_last_scale, int line_mode,
                                    int validity_rule, int keep_volumes, rslf_f2c_run** run, rslf_stats* stats, int subgrid, int peaks,
                                    float uniqueness_ratio, float propagation_ratio, float consistency_tol, int consistency_radius,
                                    int consistency_min_agree, float derivative_weight, int level_dilation, int dilation_kind,
                                    int equalize_mode, int equalize_ref_view, int equalize_joint, float equalize_max_gain) RSLF_API_TRY
{
    const F2cRequest req = {Elem::F32, h_epis, V, S, U, C, row_stride_bytes, d_min, d_max, dim_d, epi_scale_factor, p, max_pyr_depth,
                            accept_all_last_scale};
    F2cOptions o;
    o.line_mode = line_mode, o.validity_rule = validity_rule, o.keep_volumes = keep_volumes != 0, o.subgrid = subgrid;
    o.peaks = peaks, o.uniqueness = uniqueness_ratio, o.propagation_ratio = propagation_ratio;
    o.cs_tol = consistency_tol, o.cs_radius = consistency_radius, o.cs_min_agree = consistency_min_agree;
    o.derivative_weight = derivative_weight;
    o.level_dilation = level_dilation, o.dilation_kind = dilation_kind;
    o.equalize_mode = equalize_mode, o.equalize_ref_view = equalize_ref_view, o.equalize_joint = equalize_joint;
    o.equalize_max_gain = equalize_max_gain;
    return f2c_run_host(ctx, elem, req, o, run, stats);
}
RSLF_API_CATCH

// the equalisation a run was made with (each pointer nullable): mode 0, view 0 for NULL and for a run made without it; h_a_b
// [S][C][2] of the field as uploaded (C the request's: the equalisation comes before the derivative channels) is written
// only by a run made with it
extern "C" int rslf_f2c_run_equalize(const rslf_f2c_run* run, int* mode, int* ref_view, float* h_a_b) RSLF_API_TRY
{
    if (mode)
        *mode = run ? run->options.equalize_mode : 0;
    if (ref_view)
        *ref_view = run && run->options.equalize_mode ? run->options.equalize_ref_view : 0;
    if (h_a_b && run && !run->kept.view_gains.empty())
        memcpy(h_a_b, run->kept.view_gains.data(), run->kept.view_gains.size() * sizeof(float));
    return RSLF_OK;
}
RSLF_API_CATCH

// channels of the coefficients rslf_f2c_run_equalize writes: the field's own, 0 for NULL and for a run made without the equalisation
extern "C" int rslf_f2c_run_view_gains_channels(const rslf_f2c_run* run) RSLF_API_TRY
{
    return run && run->S > 0 ? (int)(run->kept.view_gains.size() / ((size_t)run->S * 2)) : 0;
}
RSLF_API_CATCH

// the level dilation a run was made with (each pointer nullable): 1 and RSLF_DILATE_CUBIC for NULL and for a run made without it
extern "C" int rslf_f2c_run_level_dilation(const rslf_f2c_run* run, int* factor, int* kind) RSLF_API_TRY
{
    if (factor)
        *factor = run ? run->options.level_dilation : 1;
    if (kind)
        *kind = run ? run->options.dilation_kind : RSLF_DILATE_CUBIC;
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_consistency_gate(const rslf_f2c_run* run, float* tol, int* radius, int* min_agree) RSLF_API_TRY
{
    if (tol)
        *tol = run ? run->options.cs_tol : 0.0f;
    if (radius)
        *radius = run ? run->options.cs_radius : 0;
    if (min_agree)
        *min_agree = run ? run->options.cs_min_agree : 0;
    return RSLF_OK;
}
RSLF_API_CATCH

// the pixels the gate made invalid on `level`; 0 on a level accepted whole and on every level of a run without the gate
extern "C" int rslf_f2c_run_inconsistent(const rslf_f2c_run* run, int level, unsigned long long* n) RSLF_API_TRY
{
    if (!run || !n)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (int rc = check_level_outside(run, level))
        return rc;
    *n = run->kept.levels[(size_t)level].inconsistent;
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" float rslf_f2c_run_propagation_ratio(const rslf_f2c_run* run)
{
    return run ? run->options.propagation_ratio : 0.0f;
}

// the sources level `level`'s sweep withheld; 0 on every level of a run without the ratio
extern "C" int rslf_f2c_run_withheld(const rslf_f2c_run* run, int level, unsigned long long* n) RSLF_API_TRY
{
    if (!run || !n)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    if (int rc = check_level_outside(run, level))
        return rc;
    *n = run->kept.levels[(size_t)level].withheld;
    return RSLF_OK;
}
RSLF_API_CATCH

// (not fields of rslf_f2c_run_desc: the structure keeps its size)
extern "C" int rslf_f2c_run_peaks(const rslf_f2c_run* run) RSLF_API_TRY
{
    return run ? run->options.peaks : 0;
}
RSLF_API_CATCH

extern "C" float rslf_f2c_run_uniqueness(const rslf_f2c_run* run)
{
    return run ? run->options.uniqueness : 0.0f;
}

// (not a field of rslf_f2c_run_desc: the structure keeps its size)
extern "C" int rslf_f2c_run_subgrid(const rslf_f2c_run* run) RSLF_API_TRY
{
    return run ? run->options.subgrid : 0;
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_destroy(rslf_f2c_run* run) RSLF_API_TRY
{
    if (!run)
        return RSLF_OK;
    (void)hipSetDevice(run->device);   // the frees wait for the device's outstanding work; no context is touched
    delete run;
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_describe(const rslf_f2c_run* run, rslf_f2c_run_desc* out) RSLF_API_TRY
{
    if (!run || !out)
        return fail(RSLF_ERR_INVALID_ARG, "run/out is NULL");
    memset(out, 0, sizeof(*out));
    const int P = (int)run->kept.levels.size();
    out->n_levels = P;
    out->S = run->S;
    out->C = run->C;
    out->device = run->device;
    out->elem = run->elem;
    out->line_mode = run->options.line_mode;
    out->validity_rule = run->options.validity_rule;
    out->keep_volumes = run->options.keep_volumes ? 1 : 0;
    std::vector<plan::LevelDims> dims;
    for (int l = 0; l < P; l++) {
        const F2cKeptLevel& kl = run->kept.levels[(size_t)l];
        out->V[l] = kl.V;
        out->U[l] = kl.U;
        out->epi_scale_factor[l] = kl.scale;
        dims.push_back(plan::LevelDims{kl.V, kl.U});
    }
    for (int which = RSLF_F2C_PLANE_DEPTH; which <= RSLF_F2C_PLANE_FUSED_LEVEL; which++) {
        size_t bytes = 0;
        if (P > 0 && plane_of(run, 0, which, &bytes))
            out->planes_held |= 1u << which;
    }
    out->device_bytes = plan::f2c_kept_bytes(run->S, run->C, dims, run->options.line_mode, run->options.keep_volumes) +
                        plan::f2c_peaks_bytes(run->options.peaks != 0, run->S, dims);
    for (int l = 0; l < P; l++) {   // the gate's planes: a gated run holds them on every level that was not accepted whole
        const bool gated = run->kept.levels[(size_t)l].cs_agree.get() != nullptr;
        if (gated)
            out->planes_held |= (1u << RSLF_F2C_PLANE_CS_AGREE) | (1u << RSLF_F2C_PLANE_CS_SEEN);
        out->device_bytes += plan::f2c_consistency_level_bytes(gated, run->S, dims[(size_t)l]);
    }
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_copy(const rslf_f2c_run* run, int level, int which, void* dst, int dst_on_host, rslf_ctx* stream_ctx) RSLF_API_TRY
{
    if (!run || !dst)
        return fail(RSLF_ERR_INVALID_ARG, "run/dst is NULL");
    if (int rc = check_level_of(run, level))
        return rc;
    if (which < RSLF_F2C_PLANE_DEPTH || which > RSLF_F2C_PLANE_CS_SEEN)
        return fail(RSLF_ERR_INVALID_ARG, "plane %d: one of RSLF_F2C_PLANE_*", which);
    if (is_fused_plane(which) && level != 0)
        return fail(RSLF_ERR_INVALID_ARG, "the fused planes are at the finest size: ask for them with level 0, not %d", level);
    if (stream_ctx && stream_ctx->device != run->device)
        return fail(RSLF_ERR_INVALID_ARG, "the run lives on device %d, the context on device %d", run->device, stream_ctx->device);
    size_t bytes = 0;
    const void* src = plane_of(run, level, which, &bytes);
    if (!src && is_peak_plane(which))
        return fail(RSLF_ERR_INVALID_ARG, "which=%d: a peak plane, and this run holds none (it was made with peaks = 0)", which);
    if (!src && is_gate_plane(which))
        return fail(RSLF_ERR_INVALID_ARG, "which=%d: a plane of the consistency gate, and level %d holds none (the run was made with "
                                          "consistency_min_agree = 0, or the level was accepted whole)", which, level);
    if (!src)
        return fail(RSLF_ERR_INVALID_ARG, "plane %d is not held by this run (C_l needs a line mode)", which);
    HIP_TRY(hipSetDevice(run->device));
    const hipMemcpyKind kind = dst_on_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (!stream_ctx) {
        HIP_TRY(hipMemcpy(dst, src, bytes, kind));
        HIP_TRY(hipDeviceSynchronize());
        return RSLF_OK;
    }
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, stream_ctx->stream));
    if (dst_on_host)
        HIP_TRY(hipStreamSynchronize(stream_ctx->stream));
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_volume(const rslf_f2c_run* run, int level, const rslf_volume** out) RSLF_API_TRY
{
    if (out)
        *out = nullptr;
    if (!run || !out)
        return fail(RSLF_ERR_INVALID_ARG, "run/out is NULL");
    if (int rc = check_level_of(run, level))
        return rc;
    const rslf_volume* vol = run->kept.levels[(size_t)level].vol.get();
    if (!vol)
        return fail(RSLF_ERR_INVALID_ARG, "the run was made without keep_volumes");
    *out = vol;
    return RSLF_OK;
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_render_depth_maps(const rslf_f2c_run* run, rslf_ctx* ctx, int saturate, const uint8_t* lut_bgr,
                                              uint8_t* d_bgr_out) RSLF_API_TRY
{
    return render_depth_maps(run, ctx, saturate, lut_bgr, d_bgr_out, false);
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_render_depth_maps_host(const rslf_f2c_run* run, rslf_ctx* ctx, int saturate, const uint8_t* lut_bgr,
                                                   uint8_t* h_bgr_out) RSLF_API_TRY
{
    return render_depth_maps(run, ctx, saturate, lut_bgr, h_bgr_out, true);
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_render_depth_pyr(const rslf_f2c_run* run, rslf_ctx* ctx, int s, int saturate, const uint8_t* lut_bgr,
                                             uint8_t* const* d_bgr_out) RSLF_API_TRY
{
    return render_depth_pyr(run, ctx, s, saturate, lut_bgr, d_bgr_out, false);
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_render_depth_pyr_host(const rslf_f2c_run* run, rslf_ctx* ctx, int s, int saturate, const uint8_t* lut_bgr,
                                                  uint8_t* const* h_bgr_out) RSLF_API_TRY
{
    return render_depth_pyr(run, ctx, s, saturate, lut_bgr, h_bgr_out, true);
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_render_epi_pyr(const rslf_f2c_run* run, rslf_ctx* ctx, int v, int saturate, const uint8_t* lut_bgr,
                                           uint8_t* const* d_bgr_out) RSLF_API_TRY
{
    return render_epi_pyr(run, ctx, v, saturate, lut_bgr, d_bgr_out, false);
}
RSLF_API_CATCH

extern "C" int rslf_f2c_run_render_epi_pyr_host(const rslf_f2c_run* run, rslf_ctx* ctx, int v, int saturate, const uint8_t* lut_bgr,
                                                uint8_t* const* h_bgr_out) RSLF_API_TRY
{
    return render_epi_pyr(run, ctx, v, saturate, lut_bgr, h_bgr_out, true);
}
RSLF_API_CATCH
