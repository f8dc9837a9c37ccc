// K4: disparity propagation of the 2-D sweep ("next" row).
//
// rslf::compute_2D_depth_epi, propagation part
// (include/rslf_depth_computation_core.hpp:1088-1129, default build: gated by the edge mask,
// :1099-1103).  For every confident pixel u of the visited view s_hat (ascending u within a
// scanline), the reference paints its disparity into every view s at column
// u + round(d * (s_hat - s) * slope) if that pixel is still in the running mask and its radiance is
// within propagation_epsilon of rbar(u); painting clears the mask, so the FIRST u (smallest) that
// qualifies wins a target pixel.  Qualifying does not depend on the order (the mask test only asks
// "not painted yet in this or an earlier visit"), so the sequential loop equals:
//   claim:  every source does atomicMin(winner[target], u) on the targets it qualifies for
//   apply:  every claimed target takes the values of its winner and leaves the mask.
// Both passes are HBM-bound streaming kernels (a few bytes per (s, v, u)).
#pragma once

#include "k_compact.hpp"
#include "k11_f2c_peak_rule.hpp"
#include "k3_median.hpp"
#include "rslf_device.hpp"

#ifndef RSLF_CLAIM_BATCH
#define RSLF_CLAIM_BATCH 8   // views whose running-mask bytes a source pixel has in flight together
#endif

namespace rslf {

constexpr int kClaimMaxViews = 1024;    // views whose "anything left to paint?" bits a claim workgroup keeps in LDS
constexpr int kNoWinner = 0x7F7F7F7F;   // what hipMemset(0x7F) leaves; >= any column index

// One source pixel's claims (core.hpp:1105-1125): `cur` is its filtered disparity.
// `live_views` (nullable; LDS, one bit per view, claim_live_views): a view none of whose segments this workgroup's sources
// can land in has a pixel left in its running mask is skipped for the whole workgroup -- after the first visits that is
// most views for most workgroups, where every source used to read one running-mask byte per view (the whole [S][V][U]
// volume, 209 MB at c3, on each of the 101 visits).
template <int C>
__device__ __forceinline__ void propagate_claim_pixel(const VolView& vol, int s_hat, int v, int u, float cur, bool source,
                                                      const float* __restrict__ rbar_vu, const uint8_t* __restrict__ mask_svu,
                                                      int* __restrict__ winner_svu, uint8_t* __restrict__ dirty, float slope,
                                                      const plan::NormThreshold& prop_thr, const unsigned long long* live_views)
{
    const int nseg = (vol.U + 255) >> 8;
    const long long o = (long long)v * vol.U + u;
    float rb[C];
#pragma unroll
    for (int c = 0; c < C; c++)
        rb[c] = source ? rbar_vu[o * C + c] : 0.0f;
    const long long plane = (long long)vol.V * vol.U;
    const long long row = (long long)v * vol.U;
    // eight views at a time: their running-mask bytes, then the radiances of those still unpainted, are loaded together
    // before the first test -- the claims do not depend on one another (atomicMin), only the loads' latency did add up
    constexpr int B = RSLF_CLAIM_BATCH;
    for (int s0 = 0; s0 < vol.S; s0 += B) {
        int ri[B];
        bool live[B];
        static_assert(64 % B == 0, "a batch of views sits in one word of the live-view bits");
        if (live_views && ((live_views[s0 >> 6] >> (s0 & 63)) & ((1ull << B) - 1ull)) == 0)
            continue;   // workgroup-uniform: nothing left to paint in these views within the workgroup's reach
        // (every load below is UNCONDITIONAL, its address clamped into the row: a load under `if (live)` sits in a basic
        // block of its own and hipcc waits for it there -- eight round trips one after the other per batch where this
        // was written to have eight in flight; k34_median_claim 217 -> 160 us per visit of a c3 sweep)
        uint8_t mb[B];
#pragma unroll
        for (int j = 0; j < B; j++) {
            const int s = s0 + j;
            // core.hpp:1109: u + (int)std::round(depth * (s_hat - s) * slope_factor)
            float off = cur * (float)(s_hat - s);
            off = off * slope;
            ri[j] = u + (int)roundf(off);
            live[j] = source && s < vol.S && ri[j] >= 0 && ri[j] < vol.U;
            ri[j] = min(max(ri[j], 0), vol.U - 1);
            mb[j] = mask_svu[(long long)min(s, vol.S - 1) * plane + row + ri[j]];
        }
        bool any = false;
#pragma unroll
        for (int j = 0; j < B; j++) {
            live[j] = live[j] && mb[j] != 0;
            any |= live[j];
        }
        if (!__any(any))
            continue;   // wave-uniform: nobody in this wave has an unpainted target in these views
        float e[B][C];
#pragma unroll
        for (int j = 0; j < B; j++) {
            // (a lane without a live target in view s0 + j reads its own column: the line its neighbours read)
            const float* er = vol.row(v, min(s0 + j, vol.S - 1));
            const int col = live[j] ? ri[j] : min(u, vol.U - 1);   // (a lane past the row's end: the last column, not the pitch's padding)
#pragma unroll
            for (int c = 0; c < C; c++)
                e[j][c] = er[col * C + c];
        }
#pragma unroll
        for (int j = 0; j < B; j++) {
            if (!live[j])
                continue;
            float df[C];
#pragma unroll
            for (int c = 0; c < C; c++)
                df[c] = e[j][c] - rb[c];
            if (norm_below<C>(df, prop_thr)) {   // core.hpp:1116: norm<T>(..) < par_propagation_epsilon
                atomicMin(&winner_svu[(long long)(s0 + j) * plane + row + ri[j]], u);
                dirty[((long long)(s0 + j) * vol.V + v) * nseg + (ri[j] >> 8)] = 1;   // this 256-column segment holds a claim
            }
        }
    }
}

// K3 + claim in one launch (a sweep visit): a pixel's median needs its neighbours' RAW depths only (what the scan
// left), and its claims need its own median only -- so the thread that filters a pixel also makes its claims.  The
// filtered plane is still written: the apply pass reads the winners' values from it.
//
// The sweep gate (rslf_sweep_propagation_ratio): the peaks mode's four [S][V][U] planes, hat = s_hat * V * U, the ratio and
// the sweep's counter of withheld sources.  A pixel that passes the gate of core.hpp:1097-1103 and whose runner-up is within
// the ratio of its winner (f2c_peak_ambiguous, the predicate of a kept pyramid's validity: one statement for both) is no
// source: it makes no claim, not even the one on itself, exactly as a pixel withheld by C_d or C_l.
struct ClaimGate {
    const int32_t* idx;
    const float* score;
    const int32_t* runner_idx;
    const float* runner_score;
    long long hat;
    float ratio;
    unsigned long long* withheld;
};

// GATED = false: `gate` is not read -- the code of a sweep without the ratio is what it was before the gate existed.
template <int C, int MODE, bool GATED>
__device__ __forceinline__ void median_claim_body(const VolView& vol, int s_hat, const float* __restrict__ raw_vu,
                                                  float* __restrict__ filtered_vu, const uint8_t* __restrict__ edge_mask_vu,
                                                  int w, const plan::NormThreshold& median_thr, const float* __restrict__ rbar_vu,
                                                  const uint8_t* __restrict__ mask_svu, int* __restrict__ winner_svu,
                                                  uint8_t* __restrict__ dirty, float slope, const plan::NormThreshold& prop_thr,
                                                  const float* __restrict__ gate_Cd_vu, float disp_thr, int* __restrict__ reset,
                                                  const int* __restrict__ remain, const ClaimGate& gate)
{
    // `reset`: the packed list's length, which the scan before this launch was the last to read and the apply pass after
    // it counts up again from 0
    if (reset && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
        *reset = 0;
    static_assert(kMedianBlock == 256, "one median tile per claim workgroup");
    extern __shared__ __attribute__((aligned(16))) float s_median_tile[];   // the window tile (k3_median.hpp)
    const int v = blockIdx.y;
    const int u_first = blockIdx.x * blockDim.x;
    const int u = u_first + threadIdx.x;
    const bool inside = u < vol.U;
    const long long o = (long long)v * vol.U + (inside ? u : vol.U - 1);
    // the pixel's peaks, four UNCONDITIONAL loads at the clamped address, in flight under the median (a load under `if`
    // waits in a block of its own: propagate_claim_pixel)
    int32_t pk_idx = -1, pk_runner_idx = -1;
    float pk_score = 0.0f, pk_runner_score = 0.0f;
    if (GATED) {
        const long long g = gate.hat + o;
        pk_idx = gate.idx[g];
        pk_runner_idx = gate.runner_idx[g];
        pk_score = gate.score[g];
        pk_runner_score = gate.runner_score[g];
    }
    // core.hpp:678-679, :881-892: the median over the edge mask, 0 elsewhere
    const float cur = selective_median_block<C, MODE>(vol, raw_vu, edge_mask_vu, s_hat, w, median_thr, v, u_first, s_median_tile);
    if (inside)
        filtered_vu[o] = cur;
    bool source = inside && (gate_Cd_vu ? gate_Cd_vu[o] > disp_thr : edge_mask_vu[o] != 0);   // core.hpp:1097-1103
    if (GATED) {
        // before the reach reduction and the workgroup's "any source?": a withheld pixel widens no reach and keeps no workgroup.
        // Counted per wave: one ballot, one vector atomic by the first lane (every lane of the workgroup is still here)
        const bool withheld = source && f2c_peak_ambiguous(pk_idx, pk_runner_idx, pk_score, pk_runner_score, gate.ratio);
        const unsigned long long b = __ballot(withheld);
        if (b != 0 && (threadIdx.x & 63) == 0)
            atomicAdd(gate.withheld, (unsigned long long)__popcll(b));
        source = source && !withheld;
    }
    // the range of the disparities the workgroup's sources hold (a non-finite one: everywhere)
    __shared__ float s_lo[4], s_hi[4];
    const bool finite = fabsf(cur) < 1.0e9f;   // false for NaN too
    float lo = source ? (finite ? cur : -1.0e9f) : INFINITY, hi = source ? (finite ? cur : 1.0e9f) : -INFINITY;
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off));
        hi = fmaxf(hi, __shfl_xor(hi, off));
    }
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
    }
    const bool any_source = __syncthreads_or(source);
    if (!any_source)
        return;
    const float cur_lo = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]));
    const float cur_hi = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
    // one thread per view decides whether the view is worth visiting at all (kClaimMaxViews views: more, and every view is visited)
    __shared__ unsigned long long s_live[kClaimMaxViews / 64];
    const bool skipping = remain != nullptr && vol.S <= kClaimMaxViews;
    if (skipping) {
        const int nseg = (vol.U + 255) >> 8;
        for (int s0 = 0; s0 < vol.S; s0 += 256) {
            const int s = s0 + threadIdx.x;
            bool any = false;
            if (s < vol.S) {
                // targets: u + round(fl(fl(cur * float(s_hat - s)) * slope)), monotone in cur; 1.5 covers the roundings
                const float k = (float)(s_hat - s) * slope;
                const float a0 = cur_lo * k, a1 = cur_hi * k;
                const int lo = max(0, (int)floorf((float)u_first + fminf(a0, a1) - 1.5f)) >> 8;
                const int hi = min(vol.U - 1, max(0, (int)ceilf((float)(u_first + 255) + fmaxf(a0, a1) + 1.5f))) >> 8;
                // eight segments' counts at a time, every load issued before the first is looked at
                const int* rr = remain + ((long long)s * vol.V + v) * nseg;
                for (int g0 = lo; g0 <= hi; g0 += 8) {
                    int r8[8];
#pragma unroll
                    for (int k = 0; k < 8; k++)
                        r8[k] = rr[min(g0 + k, hi)];
#pragma unroll
                    for (int k = 0; k < 8; k++)
                        any |= r8[k] != 0;
                }
            }
            const unsigned long long b = __ballot(any);
            if ((threadIdx.x & 63) == 0)
                s_live[(s0 + threadIdx.x) >> 6] = b;
        }
        __syncthreads();
    }
    propagate_claim_pixel<C>(vol, s_hat, v, u, cur, source, rbar_vu, mask_svu, winner_svu, dirty, slope, prop_thr, skipping ? s_live : nullptr);
}

// The kernel of every sweep without the ratio: the argument block and the code it always had.
template <int C, int MODE>
__global__ __launch_bounds__(256) void k34_median_claim(VolView vol, int s_hat, const float* __restrict__ raw_vu,
                                                       float* __restrict__ filtered_vu, const uint8_t* __restrict__ edge_mask_vu,
                                                       int w, plan::NormThreshold median_thr, const float* __restrict__ rbar_vu,
                                                       const uint8_t* __restrict__ mask_svu, int* __restrict__ winner_svu,
                                                       uint8_t* __restrict__ dirty, float slope, plan::NormThreshold prop_thr,
                                                       const float* __restrict__ gate_Cd_vu, float disp_thr, int* __restrict__ reset,
                                                       const int* __restrict__ remain)
{
    median_claim_body<C, MODE, false>(vol, s_hat, raw_vu, filtered_vu, edge_mask_vu, w, median_thr, rbar_vu, mask_svu, winner_svu, dirty,
                                      slope, prop_thr, gate_Cd_vu, disp_thr, reset, remain, ClaimGate{});
}

// ... and of a sweep with the ratio set (rslf_sweep_propagation_ratio): the same pass with the gate's planes and counter
template <int C, int MODE>
__global__ __launch_bounds__(256) void k34_median_claim_gated(VolView vol, int s_hat, const float* __restrict__ raw_vu,
                                                             float* __restrict__ filtered_vu, const uint8_t* __restrict__ edge_mask_vu,
                                                             int w, plan::NormThreshold median_thr, const float* __restrict__ rbar_vu,
                                                             const uint8_t* __restrict__ mask_svu, int* __restrict__ winner_svu,
                                                             uint8_t* __restrict__ dirty, float slope, plan::NormThreshold prop_thr,
                                                             const float* __restrict__ gate_Cd_vu, float disp_thr,
                                                             int* __restrict__ reset, const int* __restrict__ remain, ClaimGate gate)
{
    median_claim_body<C, MODE, true>(vol, s_hat, raw_vu, filtered_vu, edge_mask_vu, w, median_thr, rbar_vu, mask_svu, winner_svu, dirty,
                                     slope, prop_thr, gate_Cd_vu, disp_thr, reset, remain, gate);
}

// The apply pass of a visit (core.hpp:1119-1127) and, in the same launch, the pixel list of the NEXT visit's scan: one
// workgroup per (view, scanline) row of the planes; the rows of view s_next come first and, once their claims are
// applied (every write to a row's running mask comes from the row's own workgroup), compact that row of
// edge_mask(s_next) & running mask(s_next) into the packed list exactly as k_compact_mask_packed would have -- one dense
// pass and one launch fewer per visit.  *packed_n must be 0 on entry (k34_median_claim zeroes it: the scan before it
// was its last reader).  s_next < 0: apply only.
// `dirty` has one byte per 256-column segment of every row, set by the claims: after the first visits most segments hold
// no claim, and the pass reads the flags (S*V*ceil(U/256) bytes) instead of the winners (4 bytes per cell of the volume).
// The peaks mode's four [S][V][U] planes (rslf_sweep_peaks), each nullable: a painted pixel takes its source's values from
// the visited view's planes, as it takes C_d and C_l.  All NULL out of the mode.
struct ApplyPeaks {
    int32_t* idx;
    float* score;
    int32_t* runner_idx;
    float* runner_score;
};

// One 256-column segment of row r = s*V + v of the planes.  PEAKS = false: pk and hat are not read -- the code of a sweep
// out of the peaks mode is what it was before the mode existed.
template <bool PEAKS>
__device__ __forceinline__ void apply_segment(long long r, int seg, int V, int U, const float* __restrict__ filtered_vu,
                                              const float* __restrict__ Cd_hat_vu, float* __restrict__ depth_svu,
                                              float* __restrict__ Cd_svu, uint8_t* mask_svu, int* __restrict__ winner_svu,
                                              int* __restrict__ remain, const float* __restrict__ Cl_hat_vu,
                                              float* __restrict__ Cl_svu, const ApplyPeaks& pk, long long hat)
{
    const int u = (seg << 8) + threadIdx.x;
    const long long t = r * U + (u < U ? u : U - 1);
    const int w = u < U ? winner_svu[t] : U;
    // every claimed target was in the running mask when it was claimed and leaves it now: the segment's count follows
    const unsigned long long leaving = __ballot(w < U);
    if (remain && leaving && (threadIdx.x & 63) == 0)
        atomicSub(&remain[r * ((U + 255) >> 8) + seg], __popcll(leaving));
    if (w >= U)
        return;
    const long long src = (r % V) * U + w;     // (v, w)
    // s == s_hat: w == u, both assignments are self-assignments (core.hpp:1119-1121)
    depth_svu[t] = filtered_vu[src];
    Cd_svu[t] = Cd_hat_vu[src];
    if (Cl_svu)   // core.hpp:1122-1124: the line confidence travels with the disparity (both NULL: not kept)
        Cl_svu[t] = Cl_hat_vu[src];
    // the source's peaks, at hat + src in the same planes (hat = s_hat * V * U; self-assignments in the visited view, as above)
    if (PEAKS) {
        if (pk.idx)
            pk.idx[t] = pk.idx[hat + src];
        if (pk.score)
            pk.score[t] = pk.score[hat + src];
        if (pk.runner_idx)
            pk.runner_idx[t] = pk.runner_idx[hat + src];
        if (pk.runner_score)
            pk.runner_score[t] = pk.runner_score[hat + src];
    }
    mask_svu[t] = 0;
    winner_svu[t] = kNoWinner;
}

// remain[row][segment] = pixels of the running mask in that 256-column segment, once per sweep (rslf_sweep_begin); the
// apply passes keep it in step.  (A compaction only ever clears pixels outside the edge mask, which the running masks --
// clones of the edge masks, core.hpp:958-965 -- do not hold: should a scan drop a pixel from its edge mask, core.hpp:653-657,
// the count stays one too high, which costs a skipped skip, never a missed claim.)
__global__ __launch_bounds__(256) void k4_count_segments(const uint8_t* __restrict__ mask_svu, long long rows, int U, int* __restrict__ remain)
{
    const int nseg = (U + 255) >> 8;
    const long long item = blockIdx.x;   // one workgroup per (row, segment)
    if (item >= rows * nseg)
        return;
    const long long r = item / nseg;
    const int seg = (int)(item - r * nseg);
    const int u = (seg << 8) + threadIdx.x;
    const unsigned long long b = __ballot(u < U && mask_svu[r * U + (u < U ? u : 0)] != 0);
    __shared__ int s_n[4];
    if ((threadIdx.x & 63) == 0)
        s_n[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0)
        remain[item] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
}

constexpr int kApplyRowsPerBlock = 4;     // rows a workgroup of the general part takes (their flags: one load)
constexpr int kApplyFlagSlots = 1024;     // >= kApplyRowsPerBlock * ceil(U / 256) for U <= 65536

template <bool PEAKS>
__device__ __forceinline__ void propagate_apply_body(int S, int V, int U, int s_hat, const float* __restrict__ filtered_vu,
                                                         const float* __restrict__ Cd_hat_vu, float* __restrict__ depth_svu,
                                                         float* __restrict__ Cd_svu, uint8_t* mask_svu, int* __restrict__ winner_svu,
                                                         uint8_t* __restrict__ dirty, int s_next, const uint8_t* __restrict__ edge_mask_next_vu,
                                                         int* __restrict__ list, int* __restrict__ count,
                                                         unsigned long long* __restrict__ total, int* __restrict__ packed_n,
                                                         int* __restrict__ remain, int* __restrict__ rowbase,
                                                         const float* __restrict__ Cl_hat_vu, float* __restrict__ Cl_svu, const ApplyPeaks& pk)
{
    __shared__ uint8_t s_flags[kApplyFlagSlots];
    const long long hat = PEAKS ? (long long)s_hat * V * U : 0;
    const int nseg = (U + 255) >> 8;
    const int lead = s_next >= 0 ? V : 0;       // workgroups [0, lead): the rows of view s_next, one each
    if ((int)blockIdx.x < lead) {
        const int v = blockIdx.x;
        const long long r = (long long)s_next * V + v;
        uint8_t* flags = dirty + r * nseg;
        for (int seg = 0; seg < nseg; seg++)
            if (flags[seg])   // the same byte for the whole workgroup
                apply_segment<PEAKS>(r, seg, V, U, filtered_vu, Cd_hat_vu, depth_svu, Cd_svu, mask_svu, winner_svu, remain, Cl_hat_vu, Cl_svu, pk, hat);
        __syncthreads();      // every thread has read the flags, and this row's mask writes are the workgroup's own
        if ((int)threadIdx.x < nseg)
            flags[threadIdx.x] = 0;
        compact_row_packed(v, edge_mask_next_vu, mask_svu + (long long)s_next * V * U, U, list, count, total, packed_n, rowbase);
        return;
    }
    // every other row, kApplyRowsPerBlock at a time: one coalesced load of their flags, then only the segments that hold
    // a claim are touched
    const long long nrows = (long long)S * V;
    const long long r0 = (long long)(blockIdx.x - lead) * kApplyRowsPerBlock;
    const long long r1 = r0 + kApplyRowsPerBlock < nrows ? r0 + kApplyRowsPerBlock : nrows;
    const int nfl = (int)(r1 - r0) * nseg;
    for (int i = threadIdx.x; i < nfl; i += 256) {
        const long long r = r0 + i / nseg;
        uint8_t f = 0;
        if ((int)(r / V) != s_next) {           // the lead workgroups own those rows and their flags
            f = dirty[r0 * nseg + i];
            if (f)
                dirty[r0 * nseg + i] = 0;
        }
        s_flags[i] = f;
    }
    __syncthreads();
    for (int i = 0; i < nfl; i++)
        if (s_flags[i])
            apply_segment<PEAKS>(r0 + i / nseg, i % nseg, V, U, filtered_vu, Cd_hat_vu, depth_svu, Cd_svu, mask_svu, winner_svu, remain, Cl_hat_vu, Cl_svu, pk, hat);
}

// The kernel of every sweep out of the peaks mode: the argument block and the code it always had.
__global__ __launch_bounds__(256) void k4_propagate_apply(int S, int V, int U, int s_hat, const float* __restrict__ filtered_vu,
                                                         const float* __restrict__ Cd_hat_vu, float* __restrict__ depth_svu,
                                                         float* __restrict__ Cd_svu, uint8_t* mask_svu, int* __restrict__ winner_svu,
                                                         uint8_t* __restrict__ dirty, int s_next, const uint8_t* __restrict__ edge_mask_next_vu,
                                                         int* __restrict__ list, int* __restrict__ count,
                                                         unsigned long long* __restrict__ total, int* __restrict__ packed_n,
                                                         int* __restrict__ remain, int* __restrict__ rowbase,
                                                         const float* __restrict__ Cl_hat_vu, float* __restrict__ Cl_svu)
{
    propagate_apply_body<false>(S, V, U, s_hat, filtered_vu, Cd_hat_vu, depth_svu, Cd_svu, mask_svu, winner_svu, dirty, s_next,
                                edge_mask_next_vu, list, count, total, packed_n, remain, rowbase, Cl_hat_vu, Cl_svu, ApplyPeaks{});
}

// ... and of a sweep in the peaks mode (rslf_sweep_peaks): the same pass with the four nullable planes
__global__ __launch_bounds__(256) void k4_propagate_apply_peaks(int S, int V, int U, int s_hat, const float* __restrict__ filtered_vu,
                                                               const float* __restrict__ Cd_hat_vu, float* __restrict__ depth_svu,
                                                               float* __restrict__ Cd_svu, uint8_t* mask_svu, int* __restrict__ winner_svu,
                                                               uint8_t* __restrict__ dirty, int s_next,
                                                               const uint8_t* __restrict__ edge_mask_next_vu, int* __restrict__ list,
                                                               int* __restrict__ count, unsigned long long* __restrict__ total,
                                                               int* __restrict__ packed_n, int* __restrict__ remain, int* __restrict__ rowbase,
                                                               const float* __restrict__ Cl_hat_vu, float* __restrict__ Cl_svu, ApplyPeaks pk)
{
    propagate_apply_body<true>(S, V, U, s_hat, filtered_vu, Cd_hat_vu, depth_svu, Cd_svu, mask_svu, winner_svu, dirty, s_next,
                               edge_mask_next_vu, list, count, total, packed_n, remain, rowbase, Cl_hat_vu, Cl_svu, pk);
}

}  // namespace rslf
