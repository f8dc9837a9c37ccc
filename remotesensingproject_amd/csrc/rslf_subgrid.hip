// librslf_hip.so: the sub-grid refinement of a scan's arg max (k9_subgrid.hpp) -- rslf_subgrid_refine on planes the caller
// holds, and subgrid_refine, the launch the pile step's drivers queue between the scan and the selective median
// (rslf_pile.hip, the *_sub entries).  No score row reaches memory.  C-ABI: include/rslf_hip.h.  One device.
#include "rslf_internal.hpp"

#include "k9_subgrid.hpp"

using namespace rslf;

// Arguments checked by the caller (check_scan_args).  One launch on the context's stream; no context list, no scratch.
int rslf::subgrid_refine(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu, float dmin, float dmax,
                         int dim_d, int s_hat, const rslf_params* p, const int32_t* d_idx_vu, const float* d_score_vu, float* d_disp_vu,
                         float* d_left_vu, float* d_right_vu)
{
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
    SubgridArgs q = {};
    q.idx = d_idx_vu;
    q.score = d_score_vu;
    q.disp = d_disp_vu;
    q.left = d_left_vu;
    q.right = d_right_vu;
    const dim3 grid((vol->U + 255) / 256, vol->V), block(256);
    hipStream_t st = ctx->stream;
    const bool nearest = a.k.interp != RSLF_INTERP_LINEAR;
#define RSLF_K9_CASE(CC, CENTRE, NEAREST)                                                                          \
    if (vol->C == CC && (d_score_vu == nullptr) == CENTRE && nearest == NEAREST)                                   \
        hipLaunchKernelGGL((k9_subgrid_refine<CC, CENTRE, NEAREST>), grid, block, 0, st, a, q);
    RSLF_K9_CASE(1, false, false)
    RSLF_K9_CASE(1, true, false)
    RSLF_K9_CASE(1, false, true)
    RSLF_K9_CASE(1, true, true)
    RSLF_K9_CASE(3, false, false)
    RSLF_K9_CASE(3, true, false)
    RSLF_K9_CASE(3, false, true)
    RSLF_K9_CASE(3, true, true)
#undef RSLF_K9_CASE
    HIP_TRY(hipGetLastError());
    return RSLF_OK;
}

extern "C" int rslf_subgrid_refine(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu, float dmin,
                                   float dmax, int dim_d, int s_hat, const rslf_params* p, const int32_t* d_idx_vu,
                                   const float* d_score_vu, float* d_disp_vu, float* d_left_vu, float* d_right_vu) RSLF_API_TRY
{
    if (!ctx || !vol || !d_idx_vu || !d_disp_vu)
        return fail(RSLF_ERR_INVALID_ARG, "NULL argument");
    int rc = check_scan_args(vol, d_dmin_vu, d_dmax_vu, dim_d, s_hat, p);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return subgrid_refine(ctx, vol, d_dmin_vu, d_dmax_vu, dmin, dmax, dim_d, s_hat, p, d_idx_vu, d_score_vu, d_disp_vu, d_left_vu,
                          d_right_vu);
}
RSLF_API_CATCH
