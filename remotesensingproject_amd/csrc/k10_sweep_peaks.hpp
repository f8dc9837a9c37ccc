// K10, the peaks of a 2-D sweep's sparse visits (k10_peaks_list): winner and runner-up of every pixel a visit scanned from
// the packed list, no score row in memory.
//
// Rows for a whole sweep would be [S][V][U][D]; a sparse visit scans a few pixels per scanline, and the dense way to their
// peaks (score rows of whole windows, then k8_score_peaks) walks the plane for them.  Here a WAVE takes one entry of the
// sweep's packed list and its LANES the hypotheses, in rounds of 64: d = 64 r + lane.  Each lane scores its own hypothesis
// with scan_generic_body's operations in its order (k2_scan.hpp) -- per view the position (s_hat - s) * D * slope + u, the
// lerp of two taps (or the one tap of the nearest modes), NaN for a tap outside the row, cv::max with 0, the kernel weight,
// the sequential float sums over s, n_iter mean-shift passes, B / card -- as K9 and K7 re-run hypotheses: the scores are the
// scan's own bits whichever scan kernel made idx.  Any S, C = 1 or 3, every interpolation mode, scalar or per-pixel ranges.
//
// The peak rule (k8_peak_rule.hpp) then runs across the lanes: the candidate test of element d needs d - 1 and d + 1, two
// neighbour reads; lane 63's element waits for the next round's lane 0 (its score and its left neighbour's are carried);
// every lane folds its rounds into one (winner, runner-up) pair and a butterfly of top2_merge (k10_peak_merge.hpp,
// associative and commutative) leaves the row's pair in every lane.  Lane 0 writes the four planes.
//
// The pixel is the wave's: v, u and the EPI row base are scalars, and neighbouring lanes gather neighbouring positions of the
// same EPI rows (the positions of lanes d and d + 1 differ by (s_hat - s) * step * slope).  The taps of kPeaksListBatch
// views are issued together with clamped addresses before the first is used (K9's way).  No LDS, no atomics; a fixed grid
// strides over *packed_n entries read on the device, and nothing depends on the launch shape: every sum is sequential in s
// within one lane and the merge does not depend on its order.  An entry past the end, or one whose idx is not in
// [0, dim_d) -- a pixel the visit scanned and did not accept -- is idle.
#pragma once

#include "k2_scan.hpp"
#include "k10_peak_merge.hpp"
#include "rslf_plan_sweep_peaks.hpp"

namespace rslf {

constexpr int kPeaksListBatch = 8;   // views a lane has in flight together, one channel; three channels: half of it

struct SweepPeaksArgs {
    const int32_t* idx;        // [V][U] the visit's arg-max plane, -1: scanned and not accepted, or not scanned
    int32_t* out_idx;          // the visited view's four planes [V][U], each nullable
    float* out_score;
    int32_t* out_runner_idx;
    float* out_runner_score;
};

// The score of hypothesis Dd at pixel u of the EPI whose view 0 starts at `epi` (a scalar).  MODE: RSLF_INTERP_* at compile
// time, so that the linear kernel carries no test of the mode in its loop over the views.
template <int C, int MODE>
__device__ __forceinline__ float peaks_score_hypothesis(const ScanArgs& a, const float* __restrict__ epi, const int u, const float Dd)
{
    constexpr int N = C == 1 ? kPeaksListBatch : kPeaksListBatch / 2;
    const VolView& vol = a.vol;
    const float uf = (float)u;
    const int Um1 = vol.U - 1;
    float rbar[C];
#pragma unroll
    for (int c = 0; c < C; c++) {   // core.hpp:577, and interp.hpp:118 as built (scan_generic_body)
        rbar[c] = epi[(long long)a.s_hat * vol.stride_s + u * C + c];
        if (MODE == 2 && u != 0)
            rbar[c] = NAN;
    }
    float B = 0.0f, card = 0.0f;
    for (int it = 0; it < a.k.n_iter; it++) {
        float A[C];
#pragma unroll
        for (int c = 0; c < C; c++)
            A[c] = 0.0f;
        B = 0.0f;
        card = 0.0f;
        for (int s0 = 0; s0 < vol.S; s0 += N) {
            float e0[N][C], e1[N][C], t[N];
            bool valid[N];
#pragma unroll
            for (int j = 0; j < N; j++) {
                const int s = min(s0 + j, vol.S - 1);   // past the last view: its taps again, not used
                const float* row = epi + (long long)s * vol.stride_s;
                float x = (float)(a.s_hat - s) * Dd;   // I = S * D          core.hpp:550
                x = x * a.k.slope;                     // I *= slope_factor  core.hpp:551
                x = x + uf;                            // I += u             core.hpp:552
                const float fl = floorf(x);
                int i0 = (int)fl;                      // interp.hpp:179-181
                int ir = (int)ceilf(x);
                float w = x - fl;
                bool ok = !(i0 < 0 || ir > Um1);       // interp.hpp:182
                if (MODE != 0) {                       // one tap, weights 1 and 0 (scan_generic_body)
                    int r;
                    if (MODE == 2) {
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
                t[j] = w;
                valid[j] = ok;
#pragma unroll
                for (int c = 0; c < C; c++) {
                    e0[j][c] = row[j0 + c];
                    e1[j][c] = row[j1 + c];
                }
            }
#pragma unroll
            for (int j = 0; j < N; j++) {
                if (s0 + j >= vol.S)   // (uniform)
                    break;
                const float omt = 1.0f - t[j];
                float K;
                float R0[C];
                if (C == 1) {
                    const float m0 = omt * e0[j][0];
                    const float m1 = t[j] * e1[j][0];
                    float R = m0 + m1;                      // interp.hpp:184
                    R = valid[j] ? R : NAN;                 // interp.hpp:189
                    R0[0] = (R > 0.0f) ? R : 0.0f;          // cv::max(R, 0), NaN -> 0   core.hpp:580
                    const float delta = R - rbar[0];
                    const float qq = (a.k.k1 * delta) * delta;
                    K = kernel_weight(qq);                  // max(1 - q, 0), NaN -> 0
                } else {
                    float qc[C];
#pragma unroll
                    for (int c = 0; c < C; c++) {
                        const float m0 = omt * e0[j][c];
                        const float m1 = t[j] * e1[j][c];
                        float R = m0 + m1;
                        R = valid[j] ? R : NAN;
                        R0[c] = (R > 0.0f) ? R : 0.0f;
                        const float delta = R - rbar[c];
                        qc[c] = (a.k.inv_h2 * delta) * delta;
                    }
                    float qs = qc[0] + qc[C > 2 ? 2 : 0];   // OpenCV 3.x reduceC_: (q0 + q2) + q1
                    qs = qs + qc[C > 1 ? 1 : 0];
                    K = kernel_weight(qs);
                }
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const float pr = R0[c] * K;
                    A[c] = A[c] + pr;
                }
                B = B + K;
                card = card + (valid[j] ? 1.0f : 0.0f);
            }
        }
#pragma unroll
        for (int c = 0; c < C; c++) {
            const float m = (B != 0.0f) ? (A[c] / B) : 0.0f;   // OpenCV 3.x divide: /0 -> 0
            rbar[c] = (m > 0.0f) ? m : 0.0f;
        }
    }
    const float m = (card != 0.0f) ? (B / card) : 0.0f;   // core.hpp:620
    return (m > 0.0f) ? m : 0.0f;
}

// `a`: the scan's arguments -- volume, ranges, dim_d, s_hat, constants -- with a.list / a.packed_n the sweep's packed list
// (pixel indices v * U + u) as the visit's scan took it.
template <int C, int MODE>
__global__ __launch_bounds__(64 * plan::kPeaksListWaves) void k10_peaks_list(ScanArgs a, SweepPeaksArgs q)
{
    const unsigned n = (unsigned)max(*a.packed_n, 0);
    const int U = a.vol.U, D = a.dim_d;
    const int lane = threadIdx.x & 63;
    // (unsigned: an entry index below 2^31 plus the grid's stride, at most 2^22 waves, cannot wrap)
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * plan::kPeaksListWaves + (threadIdx.x >> 6));
    const unsigned n_waves = gridDim.x * plan::kPeaksListWaves;
    for (unsigned e = wave; e < n; e += n_waves) {
        const int px = __builtin_amdgcn_readfirstlane(a.list[e]);
        if ((unsigned)px >= (unsigned)(a.vol.V * U))   // not an entry of this plane's list: nothing is touched
            continue;
        const int i_scan = __builtin_amdgcn_readfirstlane(q.idx[px]);
        if ((unsigned)i_scan >= (unsigned)D)           // scanned and not accepted: idle
            continue;
        const int v = px / U, u = px - v * U;
        const float* epi = a.vol.row(v, 0);
        const float dmin = a.dmin_vu ? a.dmin_vu[px] : a.dmin;
        const float dmax = a.dmax_vu ? a.dmax_vu[px] : a.dmax;
        const float range = dmax - dmin;
        const float denom = (float)(D - 1);

        Top2 acc = top2_none();
        float c_prev = 0.0f, c_cur = 0.0f;   // scores of elements 64 r - 2 and 64 r - 1 once round r starts
        for (int r = 0; r * 64 < D; r++) {
            const int d = 64 * r + lane;
            const bool in = d < D;
            // (a lane past the row's end scores the last hypothesis again: uniform control flow, the value is not judged)
            const float s = peaks_score_hypothesis<C, MODE>(a, epi, u, hypothesis(dmin, range, denom, min(d, D - 1)));
            float prev = __shfl_up(s, 1);
            prev = lane == 0 ? c_cur : prev;
            const float next = __shfl_down(s, 1);
            // lane 63's element is judged now only if the row ends on it; else once the next round's lane 0 is known
            const bool now = in & ((lane != 63) | (d == D - 1));
            Top2 own = top2_one(now & is_candidate(prev, s, next, d, D), d, s);
            if (r > 0) {   // (uniform) the element carried from the round before: lane 0 takes it
                const float s_first = __shfl(s, 0);
                const int j = 64 * r - 1;
                own = top2_merge(top2_one((lane == 0) & is_candidate(c_prev, c_cur, s_first, j, D), j, c_cur), own);
            }
            acc = top2_merge(acc, own);
            c_prev = __shfl(prev, 63);
            c_cur = __shfl(s, 63);
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            Top2 o;
            o.i1 = __shfl_xor(acc.i1, off);
            o.s1 = __shfl_xor(acc.s1, off);
            o.i2 = __shfl_xor(acc.i2, off);
            o.s2 = __shfl_xor(acc.s2, off);
            acc = top2_merge(acc, o);
        }
        if (lane == 0) {
            if (q.out_idx)
                q.out_idx[px] = acc.i1;
            if (q.out_score)
                q.out_score[px] = acc.s1;
            if (q.out_runner_idx)
                q.out_runner_idx[px] = acc.i2;
            if (q.out_runner_score)
                q.out_runner_score[px] = top2_runner_score(acc);
        }
    }
}

// The dense form's mask: "this visit's idx >= 0" as the byte plane the score-row kernels and k8_score_peaks take.
__global__ __launch_bounds__(256) void k10_accepted_mask(const int32_t* __restrict__ idx, uint8_t* __restrict__ mask, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        mask[i] = idx[i] >= 0 ? 1 : 0;
}

}  // namespace rslf
