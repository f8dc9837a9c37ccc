// librslf_hip.so: the sub-grid refinement of a scan's arg max (k9_subgrid.hpp) -- rslf_subgrid_refine on planes the caller
// holds, and subgrid_refine, the launch the pile step's drivers queue between the scan and the selective median
// (rslf_pile.hip, the *_sub entries) and an open 2-D sweep in the mode queues after each visit's scan (rslf_sweep.hip), there
// over the visit's packed list where the scan took one.  No score row reaches memory.  C-ABI: include/rslf_hip.h.  One device.
#include "rslf_internal.hpp"
#include "rslf_plan_subgrid.hpp"

#include "k9_subgrid.hpp"

using namespace rslf;

// Arguments checked by the caller (check_scan_args).  One launch on the context's stream.  listed: the list form over
// Scratch::list / packed_len() as the last apply pass of the open sweep left them; else the whole plane, no context list.
int rslf::subgrid_refine(rslf_ctx* ctx, const rslf_volume* vol, const float* d_dmin_vu, const float* d_dmax_vu, float dmin, float dmax,
                         int dim_d, int s_hat, const rslf_params* p, const int32_t* d_idx_vu, const float* d_score_vu, float* d_disp_vu,
                         float* d_left_vu, float* d_right_vu, bool listed)
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
    const dim3 block(256);
    dim3 grid((vol->U + 255) / 256, vol->V);
    if (listed) {   // the sweep's packed list: its length is on the device, so a fixed grid strides over the entries
        if (!d_score_vu)
            return fail(RSLF_ERR_INTERNAL, "the list form of the sub-grid refinement takes the scan's score plane");
        if ((size_t)vol->V * vol->U > (size_t)INT32_MAX)
            return fail(RSLF_ERR_INTERNAL, "a plane of %d x %d pixels has no packed list", vol->V, vol->U);
        a.list = ctx->scratch.list.as<int>();
        a.packed_n = ctx->scratch.packed_len();
        grid = dim3(plan::subgrid_list_blocks(vol->V, vol->U, ctx->num_cus));
    }
    hipStream_t st = ctx->stream;
    const bool nearest = a.k.interp != RSLF_INTERP_LINEAR;
#define RSLF_K9_CASE(CC, CENTRE, NEAREST)                                                                          \
    if (!listed && vol->C == CC && (d_score_vu == nullptr) == CENTRE && nearest == NEAREST)                        \
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
    // the list form: a sweep's visit always holds the scan's score plane, so the winner is never scored again
#define RSLF_K9_LIST_CASE(CC, NEAREST)                                                                             \
    if (listed && vol->C == CC && nearest == NEAREST)                                                              \
        hipLaunchKernelGGL((k9_subgrid_refine_list<CC, false, NEAREST>), grid, block, 0, st, a, q);
    RSLF_K9_LIST_CASE(1, false)
    RSLF_K9_LIST_CASE(1, true)
    RSLF_K9_LIST_CASE(3, false)
    RSLF_K9_LIST_CASE(3, true)
#undef RSLF_K9_LIST_CASE
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
