// K9, sub-grid refinement (k9_subgrid_refine): a scan's arg max moved off the hypothesis grid, no score row in memory.
//
// All the sub-grid disparity of k8_peak_rule.hpp uses of a pixel's score row is the winner's score and its two neighbours'.
// The scan leaves the winner (idx, score planes); this kernel re-scores hypotheses idx - 1 and idx + 1 of every pixel -- a
// different pair in each lane, as k2_kernel_column and k7_line_confidence re-run one -- and hands the three scores to
// peak_disp, the rule k8_score_peaks applies to a whole row.  2 / dim_d of a generic scan.
//
// The scores are the scan's own bits: scan_generic_body's operations in its order (k2_scan.hpp) -- per view the position
// (s_hat - s) * D * slope + u, the lerp of two taps (or the one tap of the nearest modes), NaN for a tap outside the row,
// cv::max with 0, the kernel weight, the sequential float sums over s, n_iter mean-shift passes, B / card.  Any S, C = 1 or
// 3, negative radiances, every interpolation mode, scalar or per-pixel ranges: one kernel, whichever scan variant made idx.
//
// Work mapping: one workgroup per 256 columns of one scanline, lane = pixel (K7's).  Nothing crosses lanes and every sum is
// sequential in s, so the bits do not depend on the launch shape.  A pixel's two hypotheses (three without a score plane:
// the winner is scored too) are walked TOGETHER in one loop over s: their chains of dependent adds are independent of each
// other and fill each other's latency.  Every pass re-gathers its samples (L1 / L2 hits: neighbouring lanes read
// neighbouring floats of one EPI row); nothing is kept between passes.  The taps of kSubgridBatch views, all hypotheses, are
// issued together with clamped addresses before the first is used (kLineConfBatch's way): one memory round trip per batch
// and pass, not one per view.  No LDS, no scratch: every array below is indexed by unrolled loop counters only.
#pragma once

#include "k2_scan.hpp"
#include "k8_peak_rule.hpp"

namespace rslf {

constexpr int kSubgridBatch = 8;   // views a pixel has in flight together, one channel; three channels: half of it (the taps are registers)

struct SubgridArgs {
    const int32_t* idx;    // [V][U] the scan's arg max, -1: none
    const float* score;    // [V][U] the winner's score; NULL: the kernel scores the winner itself
    float* disp;           // [V][U] out (may be the scan's depth plane: nothing is read from it)
    float* left;           // nullable [V][U]: score of idx - 1, 0 at idx == 0
    float* right;          // nullable [V][U]: score of idx + 1, 0 at idx == dim_d - 1
};

// `a`: the scan's arguments -- volume, ranges, dim_d, s_hat, constants (the lists and output planes are not read).
// CENTRE: no score plane, the winner is the third hypothesis.  NEAREST: a.k.interp != 0, the one-tap modes (a kernel of their
// own, so that the linear one carries no test of the mode in its loop over the views).
//
// subgrid_refine_pixel is the body of one pixel (v, u), in range; both kernels below call it and nothing else touches a
// score.  In the dense kernel v is the workgroup's (the EPI base a scalar); in the list form it is the lane's.
template <int C, bool CENTRE, bool NEAREST>
__device__ __forceinline__ void subgrid_refine_pixel(const ScanArgs& a, const SubgridArgs& q, const int v, const int u)
{
    constexpr int NH = CENTRE ? 3 : 2;
    constexpr int N = C == 1 ? kSubgridBatch : kSubgridBatch / 2;
    const VolView& vol = a.vol;
    const long long o = (long long)v * vol.U + u;
    const int i1 = q.idx[o];
    if ((unsigned)i1 >= (unsigned)a.dim_d)   // -1: no disparity, nothing is touched; >= dim_d: not a scan's plane (the host cannot see it)
        return;
    const int last = a.dim_d - 1;
    const float* epi = vol.row(v, 0);
    const float uf = (float)u;
    const int Um1 = vol.U - 1;
    const float dmin = a.dmin_vu ? a.dmin_vu[o] : a.dmin;
    const float dmax = a.dmax_vu ? a.dmax_vu[o] : a.dmax;
    const float range = dmax - dmin;
    const float denom = (float)last;

    // hypothesis 0: idx - 1, 1: idx + 1, 2: idx.  At an end of the grid the missing neighbour is the winner again: scored, not used
    float Dd[NH];
    Dd[0] = hypothesis(dmin, range, denom, max(i1 - 1, 0));
    Dd[1] = hypothesis(dmin, range, denom, min(i1 + 1, last));
    if (CENTRE)
        Dd[NH - 1] = hypothesis(dmin, range, denom, i1);

    float rbar[NH][C];
#pragma unroll
    for (int c = 0; c < C; c++) {   // core.hpp:577, and interp.hpp:118 as built (scan_generic_body)
        float r0 = epi[(long long)a.s_hat * vol.stride_s + u * C + c];
        if (NEAREST && a.k.interp == 2 && u != 0)
            r0 = NAN;
#pragma unroll
        for (int h = 0; h < NH; h++)
            rbar[h][c] = r0;
    }
    float B[NH], card[NH];
#pragma unroll
    for (int h = 0; h < NH; h++)
        B[h] = card[h] = 0.0f;

    for (int it = 0; it < a.k.n_iter; it++) {
        float A[NH][C];
#pragma unroll
        for (int h = 0; h < NH; h++) {
#pragma unroll
            for (int c = 0; c < C; c++)
                A[h][c] = 0.0f;
            B[h] = 0.0f;
            card[h] = 0.0f;
        }
        for (int s0 = 0; s0 < vol.S; s0 += N) {
            float e0[N][NH][C], e1[N][NH][C], t[N][NH];
            bool valid[N][NH];
#pragma unroll
            for (int j = 0; j < N; j++) {
                const int s = min(s0 + j, vol.S - 1);   // past the last view: its taps again, not used
                const float* row = epi + (long long)s * vol.stride_s;
                const float sf = (float)(a.s_hat - s);
#pragma unroll
                for (int h = 0; h < NH; h++) {
                    float x = sf * Dd[h];                  // I = S * D          core.hpp:550
                    x = x * a.k.slope;                     // I *= slope_factor  core.hpp:551
                    x = x + uf;                            // I += u             core.hpp:552
                    const float fl = floorf(x);
                    int i0 = (int)fl;                      // interp.hpp:179-181
                    int ir = (int)ceilf(x);
                    float w = x - fl;
                    bool ok = !(i0 < 0 || ir > Um1);       // interp.hpp:182
                    if (NEAREST) {                         // one tap, weights 1 and 0 (scan_generic_body)
                        int r;
                        if (a.k.interp == 2) {
                            r = __float_as_int(x);         // interp.hpp:118
                            ok = r > -1 && r < vol.U;      // interp.hpp:122
                        } else {
                            r = (int)roundf(x);            // interp.hpp:121
                            ok = fabsf(x) < 2.0e9f && r > -1 && r < vol.U;
                        }
                        i0 = ir = r;
                        w = 0.0f;
                    }
                    // (unsigned element offsets from the view's row, a uniform pointer: 32-bit address arithmetic per tap)
                    const unsigned j0 = (unsigned)min(max(i0, 0), Um1) * C, j1 = (unsigned)min(max(ir, 0), Um1) * C;
                    t[j][h] = w;
                    valid[j][h] = ok;
#pragma unroll
                    for (int c = 0; c < C; c++) {
                        e0[j][h][c] = row[j0 + c];
                        e1[j][h][c] = row[j1 + c];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < N; j++) {
                if (s0 + j >= vol.S)   // (uniform)
                    break;
#pragma unroll
                for (int h = 0; h < NH; h++) {
                    const float omt = 1.0f - t[j][h];
                    float K;
                    float R0[C];
                    if (C == 1) {
                        const float m0 = omt * e0[j][h][0];
                        const float m1 = t[j][h] * e1[j][h][0];
                        float R = m0 + m1;                      // interp.hpp:184
                        R = valid[j][h] ? R : NAN;              // interp.hpp:189
                        R0[0] = (R > 0.0f) ? R : 0.0f;          // cv::max(R, 0), NaN -> 0   core.hpp:580
                        const float delta = R - rbar[h][0];
                        const float qq = (a.k.k1 * delta) * delta;
                        K = kernel_weight(qq);                  // max(1 - q, 0), NaN -> 0
                    } else {
                        float qc[C];
#pragma unroll
                        for (int c = 0; c < C; c++) {
                            const float m0 = omt * e0[j][h][c];
                            const float m1 = t[j][h] * e1[j][h][c];
                            float R = m0 + m1;
                            R = valid[j][h] ? R : NAN;
                            R0[c] = (R > 0.0f) ? R : 0.0f;
                            const float delta = R - rbar[h][c];
                            qc[c] = (a.k.inv_h2 * delta) * delta;
                        }
                        float qs = qc[0] + qc[C > 2 ? 2 : 0];   // OpenCV 3.x reduceC_: (q0 + q2) + q1
                        qs = qs + qc[C > 1 ? 1 : 0];
                        K = kernel_weight(qs);
                    }
#pragma unroll
                    for (int c = 0; c < C; c++) {
                        const float pr = R0[c] * K;
                        A[h][c] = A[h][c] + pr;
                    }
                    B[h] = B[h] + K;
                    card[h] = card[h] + (valid[j][h] ? 1.0f : 0.0f);
                }
            }
        }
#pragma unroll
        for (int h = 0; h < NH; h++) {
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float m = (B[h] != 0.0f) ? (A[h][c] / B[h]) : 0.0f;   // OpenCV 3.x divide: /0 -> 0
                rbar[h][c] = (m > 0.0f) ? m : 0.0f;
            }
        }
    }
    float sc[NH];
#pragma unroll
    for (int h = 0; h < NH; h++) {
        const float m = (card[h] != 0.0f) ? (B[h] / card[h]) : 0.0f;   // core.hpp:620
        sc[h] = (m > 0.0f) ? m : 0.0f;
    }
    const float s1 = CENTRE ? sc[NH - 1] : q.score[o];
    q.disp[o] = peak_disp(i1, a.dim_d, dmin, dmax, sc[0], s1, sc[1]);
    if (q.left)
        q.left[o] = i1 == 0 ? 0.0f : sc[0];
    if (q.right)
        q.right[o] = i1 == last ? 0.0f : sc[1];
}

template <int C, bool CENTRE, bool NEAREST>
__global__ __launch_bounds__(256) void k9_subgrid_refine(ScanArgs a, SubgridArgs q)
{
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= a.vol.U)
        return;
    subgrid_refine_pixel<C, CENTRE, NEAREST>(a, q, blockIdx.y, u);
}

// The list-driven form: lane = entry of a 2-D sweep's packed list (a.list: pixel indices v * U + u, row-contiguous,
// ascending u; a.packed_n: its length, known to the device alone).  After the centre view a visit scans a few pixels per
// scanline; over the whole plane nearly every wave of the dense kernel would still hold one live lane and walk all the
// sample passes for it.  Here 64 consecutive entries make a wave -- mostly one scanline's, neighbours in u, so their taps
// share cache lines as a row's do -- and each lane carries its own row pointer.  A fixed grid strides over the entries (no
// host read of the length); a lane past the end, or whose idx is not in [0, dim_d), does nothing.  Same body, nothing
// crosses lanes: the bits are the dense kernel's whatever the mapping.  No LDS, no scratch.
template <int C, bool CENTRE, bool NEAREST>
__global__ __launch_bounds__(256) void k9_subgrid_refine_list(ScanArgs a, SubgridArgs q)
{
    const unsigned n = (unsigned)max(*a.packed_n, 0);
    const int U = a.vol.U;
    // (unsigned: an entry index below 2^31 plus the grid's stride, at most 2^22 lanes, cannot wrap)
    for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const int px = a.list[e];
        if ((unsigned)px >= (unsigned)(a.vol.V * U))   // not an entry of this plane's list: nothing is touched
            continue;
        subgrid_refine_pixel<C, CENTRE, NEAREST>(a, q, px / U, px % U);
    }
}

}  // namespace rslf
