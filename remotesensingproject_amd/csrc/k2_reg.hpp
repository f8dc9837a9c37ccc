// K2, register variant (k2_scan_reg / k2_scan_reg_packed): every sample of a unit held in registers.
// Common definitions, work mapping and the epilogue: k2_scan.hpp.
#pragma once

#include "k2_scan.hpp"
#include "k2_taps.hpp"

namespace rslf {

// ---------------------------------------------------------------------------
// Register variant: C*SPAD sample registers, every radiance in [0, 1e6].
//
// The S samples (x C channels) of one (pixel, hypothesis) are gathered once into
// VGPRs and the mean-shift passes run out of registers, no memory instruction:
//   C = 1:  delta = R - rbar ; t = k1*delta ; q = t*delta ; K = clamp(1 - q)
//           P = R*K ; A += P ; B += K                                  ( 7 VALU / sample / pass)
//   C = 3:  per channel delta, t = inv_h2*delta, q = t*delta ; qs = (q0+q2)+q1 ; K = clamp(1 - qs)
//           per channel P = R*K, A += P ; B += K                       (19 VALU / sample / pass)
// Out-of-range samples (the reference's NaN, interp.hpp:189) and the padding
// slots s >= S hold kSentinel = 1e30 in every channel: then q = +inf, K = max(-inf, 0) = 0
// and P = 1e30 * 0 = 0 exactly, so they add +0 to every sum -- bit-identical to the
// reference's "NaN -> K = 0, R0 = 0" without a second register per sample.
// Needs R == max(R, 0), hence the non-negative-volume precondition checked by
// the host (rslf_plan.hpp: choose_scan_kernel).
// ---------------------------------------------------------------------------
// samples whose loads are in flight together (2 registers per sample and channel while they are)
#ifndef RSLF_REG_GB104
#define RSLF_REG_GB104 8    // loads in flight per gather round of the 104-slot (c3) kernel.  8: no scratch, HBM traffic 1.03x the
                            // algorithmic bytes.  13 (eight rounds per hypothesis instead of thirteen; round 3's default) is 0.86 % faster
                            // -- four same-box alternations, 65.67-65.84 vs 66.24-66.41 ms -- at the price of 28 B/lane of per-tile
                            // scratch that reaches HBM: 1.41x the algorithmic bytes.  Below the 1 % bar: the scratch-free build ships
                            // (profiles/r04_k2_variants.md).
#endif
constexpr int gather_batch(int c) { return c == 1 ? 8 : 4; }
constexpr int kPadSlack = 16;     // compiled slot counts step by at most this: only the last kPadSlack slots can be padding

// One mean-shift pass over the samples of a (pixel, hypothesis) unit held in registers: A[c] += R*K, B += K in ascending s
// (core.hpp:589-606).  KONLY: B alone -- the last pass of a TRIM scan (A is left untouched).
template <int SPAD, int C, bool PK, bool KONLY>
__device__ __forceinline__ void mean_shift_pass(const float (&R)[PK ? 1 : C][PK ? 1 : SPAD], const f2 (&R2)[PK ? C : 1][PK ? SPAD / 2 : 1],
                                                int S, float kq, const float (&rbar)[C], float (&A)[C], float& B)
{
    static_assert(!KONLY || (C == 1 && !PK), "the K-only pass is written for the scalar one-channel blocks");
    if constexpr (PK) {
        // a pair of samples per step: delta, kq*delta, q, K and R*K as packed instructions on both
        // samples, then the sums take sample s and sample s+1 in turn (core.hpp:602-603 order)
        f2 rb2[C];
        const f2 kq2 = {kq, kq};
#pragma unroll
        for (int c = 0; c < C; c++)
            rb2[c] = f2{rbar[c], rbar[c]};
        // hand-scheduled blocks of 8 (C = 1) / 4 (C = 3) samples; the slots of a block that lie beyond S are
        // padding (K = P = +0 exactly), whole blocks beyond S are skipped (wave-uniform)
        constexpr int kBlk = (C == 1) ? 8 : 4;
#pragma unroll
        for (int s0 = 0; s0 < SPAD; s0 += kBlk) {
            if (!(s0 < SPAD - kPadSlack || s0 < S))
                continue;
            if constexpr (C == 1) {
                f2 P[4], K[4];
                const f2 r4[4] = {R2[0][s0 / 2], R2[0][s0 / 2 + 1], R2[0][s0 / 2 + 2], R2[0][s0 / 2 + 3]};
                mean_shift_pk_octet(r4, rb2[0], kq2, P, K);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    A[0] = A[0] + P[j].x;                // core.hpp:602, ascending s
                    B = B + K[j].x;                      // core.hpp:603
                    A[0] = A[0] + P[j].y;
                    B = B + K[j].y;
                }
            } else {
                f2 Pa[3], Pb[3], Ka, Kb;
                const f2 ra[3] = {R2[0][s0 / 2], R2[1][s0 / 2], R2[C - 1][s0 / 2]};
                const f2 rb[3] = {R2[0][s0 / 2 + 1], R2[1][s0 / 2 + 1], R2[C - 1][s0 / 2 + 1]};
                const f2 m[3] = {rb2[0], rb2[C > 1 ? 1 : 0], rb2[C - 1]};
                mean_shift_pk_rgb_quad(ra, rb, m, kq2, Pa, Pb, Ka, Kb);
#pragma unroll
                for (int c = 0; c < C; c++)
                    A[c] = A[c] + Pa[c].x;
                B = B + Ka.x;
#pragma unroll
                for (int c = 0; c < C; c++)
                    A[c] = A[c] + Pa[c].y;
                B = B + Ka.y;
#pragma unroll
                for (int c = 0; c < C; c++)
                    A[c] = A[c] + Pb[c].x;
                B = B + Kb.x;
#pragma unroll
                for (int c = 0; c < C; c++)
                    A[c] = A[c] + Pb[c].y;
                B = B + Kb.y;
            }
        }
    } else if (C == 1) {
        // hand-scheduled, four samples per block (rslf_device.hpp).  Only the last kPadSlack slots can
        // be padding: there a wave-uniform test skips what lies beyond S (a padded slot would add +0
        // to both sums, so skipping it changes nothing but the instruction count).
#pragma unroll
        for (int s0 = 0; s0 < SPAD; s0 += 4) {
            if (s0 + 4 <= SPAD - kPadSlack || s0 + 4 <= S) {
                if constexpr (KONLY)
                    mean_shift_group4_k(R[0][s0], R[0][s0 + 1], R[0][s0 + 2], R[0][s0 + 3], rbar[0], kq, B);
                else
                    mean_shift_group4(R[0][s0], R[0][s0 + 1], R[0][s0 + 2], R[0][s0 + 3], rbar[0], kq, A[0], B);
            } else {
#pragma unroll
                for (int j = 0; j < 3; j++)
                    if (s0 + j < S) {
                        if constexpr (KONLY)
                            mean_shift_group1_k(R[0][s0 + j], rbar[0], kq, B);
                        else
                            mean_shift_group1(R[0][s0 + j], rbar[0], kq, A[0], B);
                    }
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < SPAD; s++) {
            if (!(s < SPAD - kPadSlack || s < S))   // wave-uniform: padding slot
                continue;
            float q[C];
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float delta = R[c][s] - rbar[c];   // core.hpp:591
                const float tq = kq * delta;             // kernels.cpp:21 / :43
                q[c] = tq * delta;
            }
            float qs = q[0];
            if (C == 3) {
                qs = q[0] + q[C - 1];                    // OpenCV 3.x reduceC_: (q0 + q2) + q1
                qs = qs + q[C > 1 ? 1 : 0];
            }
            const float K = kernel_weight(qs);           // kernels.cpp:23-25 / :51-53
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float pr = R[c][s] * K;            // core.cpp:28 / :36
                A[c] = A[c] + pr;                        // core.hpp:602
            }
            B = B + K;                                   // core.hpp:603
        }
    }
}

// One gather batch of the row form with a tap table (scan_reg_body, TAPS).  `from_table` (wave-uniform): the tile's pixels
// are consecutive, every slot of the batch holds a sample and each has an entry that serves every lane -- address and
// weights are the entry's, one address add per sample.  Otherwise they are computed per lane, as scan_reg_body does
// without a table.  Both forms feed ONE copy of the loads and the blend: what meets after the branch are the batch's
// short-lived addresses and weights, not the sample registers (two copies of the blend put those in scratch).
// Interior hypotheses only: every sample is inside the row, so there is no validity to carry.  (The border form was built
// as well: validity then meets after the branch as a register and costs the per-lane batches two instructions per sample.)
template <int SPAD, int C, int BATCH>
__device__ __forceinline__ void tap_table_batch(const float* epi, const float* otab, const int* tboff, const f2* tw, unsigned du_bytes,
                                                float uf, int S, int stride_s, bool from_table, int g, int& rowoff, float (&R)[C][SPAD])
{
    float tt[BATCH], om[BATCH], e0[C][BATCH], e1[C][BATCH];
    unsigned bo[BATCH];
    if (from_table) {
#pragma unroll
        for (int j = 0; j < BATCH; j++) {
            const int s = g * BATCH + j;
            bo[j] = (unsigned)tboff[s] + du_bytes;
            const f2 w = tw[s];   // (t, 1 - t)
            tt[j] = w.x;
            om[j] = w.y;
        }
    } else {
        int ro = rowoff;
#pragma unroll
        for (int j = 0; j < BATCH; j++) {
            const int s = g * BATCH + j;
            tt[j] = 0.0f;
            bo[j] = 0;
            if (s < SPAD - kPadSlack || s < S) {
                const float x = otab[s] + uf;      // core.hpp:552
                tt[j] = lerp_weight(x);            // interp.hpp:181
                const int i0 = floor_to_int(x);    // interp.hpp:179
                bo[j] = (unsigned)(i0 * C + ro) << 2;
            }
            om[j] = 1.0f - tt[j];
            ro += stride_s;
        }
    }
    rowoff += BATCH * stride_s;
    // the batch's loads back to back, then the blend
#pragma unroll
    for (int j = 0; j < BATCH; j++) {
        const int s = g * BATCH + j;
#pragma unroll
        for (int c = 0; c < C; c++) {
            e0[c][j] = kSentinel;
            e1[c][j] = 0.0f;
        }
        if (s < SPAD - kPadSlack || s < S) {
            const float* p = (const float*)((const char*)epi + bo[j]);
#pragma unroll
            for (int c = 0; c < C; c++) {
                e0[c][j] = p[c];
                e1[c][j] = p[C + c];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < BATCH; j++) {
        const int s = g * BATCH + j;
#pragma unroll
        for (int c = 0; c < C; c++) {
            const float m0 = om[j] * e0[c][j];   // interp.hpp:184
            const float m1 = tt[j] * e1[c][j];
            const float r = m0 + m1;
            R[c][s] = (s < SPAD - kPadSlack || s < S) ? r : kSentinel;
        }
    }
}

// BORDER:    some sample line of this wave may leave [0, U-1]: test validity per sample.
// UNIFORM_D: every pixel shares the hypothesis grid (no per-pixel dmin/dmax planes), so the
//            view offset fl(fl(float(s_hat - s) * D[d]) * slope) is the same for all 64 lanes:
//            the wave computes the S offsets of a hypothesis once (2-4 lane-parallel rounds),
//            parks them in LDS and every sample starts from one broadcast ds_read -- 3 VALU
//            instructions fewer per sample than recomputing them per lane.
// PK:        the samples live in register PAIRS (s, s+1) and the mean-shift pass uses packed fp32
//            instructions on them; the sums still take one sample at a time, in ascending s.  For the
//            variants that run at one wave per SIMD (rslf_device.hpp, f2).
// GB:        samples whose loads are in flight together, 0 = the default (gather_batch).  The packed kernel of long
//            one-channel units asks for a quarter of the unit at once: on a sparse launch a wave has its SIMD nearly to
//            itself, and a hypothesis costs it one memory round trip per batch.
// LANE_D:    the lanes of the wave own HYPOTHESES of one pixel instead of pixels (k2_scan_reg_px): lane `dlane` scores
//            d0 + dlane, d0 + dlane + dstep, ... below d1 (a lane past the end repeats d1 - 1 and offers nothing).
// TRIM:      the last mean-shift pass sums K alone (the score) and `best` is offered the rbar that ENTERED it; the
//            kernel's epilogue recomputes the last pass for the winning hypothesis of each pixel (last_pass_rbar).
// TAPS:      (with UNIFORM_D) the lanes that compute the view offsets also compute, per offset, the tap entry of the whole
//            tile (k2_taps.hpp): {address of the first pixel's left tap, t, 1 - t} and whether it holds for every lane.
//            `otab` is then three tables in 4 * SPAD floats, [offsets][addresses][(t, 1 - t) pairs].  On a tile of consecutive pixels a
//            gather batch whose samples all have such an entry takes them from it: per sample one address add and the
//            blend -- no position add, fract, floor-convert, address shift or 1 - t, which give the same bits in every lane.
//            Every other batch runs the per-lane form.
template <int SPAD, int C, bool BORDER, bool UNIFORM_D, bool PK, int GB = 0, class BestT = Best<C>, bool LANE_D = false,
          bool TRIM = false, bool TAPS = false>
__device__ __forceinline__ void scan_reg_body(const ScanArgs& a, int v, int u, int d0, int d1, BestT& best,
                                              float* __restrict__ otab, int dlane = 0, int dstep = 1)
{
    static_assert(!LANE_D || !UNIFORM_D, "hypotheses in the lanes: every lane has its own view offsets");
    // 104 slots (the c3 shape) have 15 registers to spare at three waves per SIMD: 13 loads in flight instead of 8
    // (8 batches instead of 13 per hypothesis) measured 0.5 % faster
    constexpr int kGatherBatch = GB > 0 ? GB : (C == 1 && !PK && SPAD == 104 && RSLF_REG_GB104 == 13) ? 13 : gather_batch(C);
    static_assert(SPAD % kGatherBatch == 0 && (!PK || kGatherBatch % 2 == 0), "whole batches, whole pairs");
    static_assert(SPAD % 8 == 0, "slot counts are multiples of 8");
    static_assert(!TAPS || (UNIFORM_D && !BORDER && !PK), "the tap table belongs to the interior scalar uniform-D row form");
    const VolView& vol = a.vol;
    const float* epi = vol.row(v, 0);
    const float uf = (float)u;
    const int Um1 = vol.U - 1;
    const unsigned Um1_bits = __float_as_uint((float)Um1);
    const int S = vol.S;
    const int lane = threadIdx.x & 63;
    const long long o = (long long)v * vol.U + u;
    const float dmin = a.dmin_vu ? a.dmin_vu[o] : a.dmin;
    const float dmax = a.dmax_vu ? a.dmax_vu[o] : a.dmax;
    const float range = dmax - dmin;
    const float denom = (float)(a.dim_d - 1);
    const float kq = (C == 1) ? a.k.k1 : a.k.inv_h2;   // kernels.cpp:21 / :43
    const float slope = a.k.slope;
    const int stride_s = (int)vol.stride_s;
    // core.hpp:577: rbar starts from R[s_hat] = E[s_hat][u] for every hypothesis
    float centre[C];
#pragma unroll
    for (int c = 0; c < C; c++)
        centre[c] = epi[(long long)a.s_hat * vol.stride_s + u * C + c];
    // TAPS: the tile's first and last pixel (idle lanes shadow the last one, scan_tile), this lane's place among them as
    // a byte offset, and whether the lanes hold consecutive pixels -- all the table's entries assume
    int* const tboff = TAPS ? reinterpret_cast<int*>(otab + SPAD) : nullptr;
    f2* const tw = TAPS ? reinterpret_cast<f2*>(otab + 2 * SPAD) : nullptr;
    int u_first = 0, u_last = 0;
    unsigned du_bytes = 0;
    bool taps_on = false;
    if constexpr (TAPS) {
        u_first = __builtin_amdgcn_readfirstlane(u);
        u_last = __builtin_amdgcn_readlane(u, 63);
        const int du = u - u_first;
        du_bytes = (unsigned)(du * C) << 2;
        taps_on = a.tap_table != 0 && __all(du == min(lane, u_last - u_first));
    }

#pragma unroll 1
    for (int dk = d0; dk < d1; dk += (LANE_D ? dstep : 1)) {
        const int d = LANE_D ? min(dk + dlane, d1 - 1) : dk;
        const float Dd = hypothesis(dmin, range, denom, d);
        float R[PK ? 1 : C][PK ? 1 : SPAD];
        f2 R2[PK ? C : 1][PK ? SPAD / 2 : 1];
        int card = BORDER ? 0 : S;
        // The gather is fully unrolled (R[] must be register-indexed).  Everything in it that
        // does not depend on d would otherwise be hoisted out of the d loop -- SPAD row
        // pointers and SPAD float(s_hat - s) values pinned in registers for the whole kernel.
        // Two values re-made opaque per hypothesis keep that state to two registers: the
        // view offset of s = 0 as a float, and the running row offset.
        float Ss0 = (float)a.s_hat;
        asm volatile("" : "+v"(Ss0));
        int rowoff = 0;
        asm volatile("" : "+s"(rowoff));
        unsigned fastb = 0;   // TAPS: bit g = gather batch g takes its samples from the tap table
        if (UNIFORM_D) {
            // (TAPS: what the entries are made from is re-made opaque per hypothesis like the address state above, so that
            // nothing of it stays in registers through the passes)
            int lane_s = lane, tile_first = u_first, tile_last = u_last;
            if constexpr (TAPS)
                asm volatile("" : "+v"(lane_s), "+s"(tile_first), "+s"(tile_last));
#pragma unroll
            for (int s0 = 0; s0 < SPAD; s0 += 64) {
                const int s = s0 + lane_s;
                float off = (float)(a.s_hat - s) * Dd;   // float(s_hat - s) * D[d]   core.hpp:542,550
                off = off * slope;                       // core.hpp:551
                if (SPAD % 64 == 0 || s < SPAD)
                    otab[s] = off;
                if constexpr (TAPS) {
                    if (taps_on) {   // (wave-uniform)
                        const TapEntry e = tap_entry(off, tile_first, tile_last, vol.U, C, __mul24(s, stride_s));
                        if (SPAD % 64 == 0 || s < SPAD) {
                            tboff[s] = e.byteoff;
                            tw[s] = f2{e.t, e.omt};
                        }
                        // bit 8 k of m: the eight samples from s0 + 8 k on all have an entry for the whole tile
                        unsigned long long m = __ballot(e.fast);
                        m &= m >> 1;
                        m &= m >> 2;
                        m &= m >> 4;
                        static_assert(!TAPS || kGatherBatch == 8, "the batch bits are gathered for batches of eight samples");
#pragma unroll
                        for (int k = 0; k < 8; k++)
                            if (s0 + 8 * k < SPAD)
                                fastb |= ((unsigned)(m >> (8 * k)) & 1u) << (s0 / 8 + k);
                    }
                }
            }
            // same wave, LDS is in order: the broadcast reads below see these writes
            __builtin_amdgcn_wave_barrier();
            if constexpr (TAPS)   // whole batches only: the one that reaches past S has padding slots
                fastb = __builtin_amdgcn_readfirstlane(fastb & (S >= SPAD ? ~0u : (1u << (S / kGatherBatch)) - 1u));
        }
#pragma unroll
        for (int g = 0; g < SPAD / kGatherBatch; g++) {
            if constexpr (TAPS) {
                tap_table_batch<SPAD, C, kGatherBatch>(epi, otab, tboff, tw, du_bytes, uf, S, stride_s, (fastb >> g) & 1u, g, rowoff, R);
            } else {
                float tt[kGatherBatch], e0[C][kGatherBatch], e1[C][kGatherBatch];
                bool ok[kGatherBatch];
                // issue the batch's loads back to back, then blend
#pragma unroll
                for (int j = 0; j < kGatherBatch; j++) {
                    const int s = g * kGatherBatch + j;
                    tt[j] = 0.0f;
                    ok[j] = false;
#pragma unroll
                    for (int c = 0; c < C; c++) {
                        e0[c][j] = kSentinel;
                        e1[c][j] = 0.0f;
                    }
                    if (s < SPAD - kPadSlack || s < S) {
                        float x;
                        if (UNIFORM_D) {
                            x = otab[s];                   // one broadcast read for the wave
                        } else {
                            x = (Ss0 - (float)s) * Dd;     // float(s_hat - s) * D[d]   core.hpp:542,550
                            x = x * slope;                 // core.hpp:551
                        }
                        x = x + uf;                        // core.hpp:552
                        tt[j] = lerp_weight(x);            // interp.hpp:181
                        int i0 = floor_to_int(x);          // interp.hpp:179
                        ok[j] = true;
                        if (BORDER) {
                            // interp.hpp:182: floor(x) >= 0 <=> x >= 0 and ceil(x) <= U-1 <=> x <= U-1.
                            // x is never -0 (u >= +0 is added last), so both tests are ONE unsigned compare
                            // of the bit patterns: negative floats have the sign bit set and compare high.
                            ok[j] = __float_as_uint(x) <= Um1_bits;
                            i0 = ok[j] ? i0 : 0;           // keep the address inside the row
                        }
                        // 32-bit byte offset off the EPI's scalar base
                        const unsigned byteoff = (unsigned)(i0 * C + rowoff) << 2;
                        // both taps of every channel are 2*C consecutive floats of the row (interleaved slab).  For
                        // integral x the reference reads the first tap twice with weights 1 and 0; 0 * (second tap)
                        // is the same +0 (rows are zero padded, so the second tap is finite)
                        const float* p = (const float*)((const char*)epi + byteoff);
#pragma unroll
                        for (int c = 0; c < C; c++) {
                            e0[c][j] = p[c];
                            e1[c][j] = p[C + c];
                        }
                    }
                    rowoff += stride_s;
                }
#pragma unroll
                for (int j = 0; j < kGatherBatch; j++) {
                    const int s = g * kGatherBatch + j;
                    const float omt = 1.0f - tt[j];
#pragma unroll
                    for (int c = 0; c < C; c++) {
                        const float m0 = omt * e0[c][j];   // interp.hpp:184
                        const float m1 = tt[j] * e1[c][j];
                        const float r = m0 + m1;
                        float val;
                        if (BORDER)
                            val = ok[j] ? r : kSentinel;
                        else
                            val = (s < SPAD - kPadSlack || s < S) ? r : kSentinel;
                        if constexpr (PK) {
                            if (s & 1)
                                R2[c][s >> 1].y = val;
                            else
                                R2[c][s >> 1].x = val;
                        } else {
                            R[c][s] = val;
                        }
                    }
                    if (BORDER)
                        card += ok[j] ? 1 : 0;
                }
            }
            // Pin this batch: its results must exist here, and the next batch's address state is
            // re-made opaque here, so the compiler cannot turn the unrolled gather into "all
            // loads first, all blends last" (which parks 2*C*SPAD loaded values in scratch).
            {
                const int b = g * kGatherBatch;
#pragma unroll
                for (int c = 0; c < C; c++) {
                    if constexpr (PK) {
                        asm volatile("" : "+v"(R2[c][b / 2]), "+v"(R2[c][b / 2 + 1]));
                        if (kGatherBatch == 8)
                            asm volatile("" : "+v"(R2[c][b / 2 + 2]), "+v"(R2[c][b / 2 + 3]));
                        static_assert(!PK || kGatherBatch == 4 || kGatherBatch == 8, "pair pinning is written for 4 and 8");
                    } else if (kGatherBatch != 4 && kGatherBatch != 8) {
#pragma unroll
                        for (int j = 0; j < kGatherBatch; j++)
                            asm volatile("" : "+v"(R[c][b + j]));
                    } else {
                        asm volatile("" : "+v"(R[c][b + 0]), "+v"(R[c][b + 1]), "+v"(R[c][b + 2]), "+v"(R[c][b + 3]));
                        if (kGatherBatch == 8)
                            asm volatile("" : "+v"(R[c][b + kGatherBatch - 4]), "+v"(R[c][b + kGatherBatch - 3]),
                                              "+v"(R[c][b + kGatherBatch - 2]), "+v"(R[c][b + kGatherBatch - 1]));
                    }
                }
                if (BORDER)
                    asm volatile("" : "+s"(rowoff), "+v"(Ss0), "+v"(card));
                else
                    asm volatile("" : "+s"(rowoff), "+v"(Ss0));
            }
        }

        float rbar[C];
#pragma unroll
        for (int c = 0; c < C; c++)
            rbar[c] = centre[c];
        float B = 0.0f;
#pragma unroll 1
        for (int it = 0; it < a.k.n_iter; it++) {   // core.hpp:584-610
            float A[C];
#pragma unroll
            for (int c = 0; c < C; c++)
                A[c] = 0.0f;
            B = 0.0f;
            if constexpr (TRIM) {
                if (it == a.k.n_iter - 1) {
                    // the last pass sums K alone, and rbar stays the one that entered it (LastPassRbar)
                    mean_shift_pass<SPAD, C, PK, true>(R, R2, S, kq, rbar, A, B);
                    break;
                }
            }
            mean_shift_pass<SPAD, C, PK, false>(R, R2, S, kq, rbar, A, B);
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float qd = (B != 0.0f) ? (A[c] / B) : 0.0f;   // core.cpp:42 / :50, OpenCV 3.x: /0 -> 0
                rbar[c] = (qd > 0.0f) ? qd : 0.0f;                  // core.hpp:609
            }
        }
        const float cardf = (float)card;
        float sc = (card != 0) ? (B / cardf) : 0.0f;   // core.hpp:616-620: the last pass's sum of K
        sc = (sc > 0.0f) ? sc : 0.0f;                  // core.hpp:622
        if (!LANE_D || dk + dlane < d1)
            best.offer(sc, d, Dd, rbar);
    }
}

// The last mean-shift pass of ONE (pixel, hypothesis), from the rbar that entered it: what a TRIM scan leaves out for every
// hypothesis but the winner.  The samples are gathered again with scan_reg_body's per-lane arithmetic (the uniform-D
// offset table holds the same values: float(s_hat) - float(s) is float(s_hat - s) exactly), out-of-range ones are
// kSentinel, and the pass is mean_shift_pass's: the K values are those whose sum is the stored score's numerator, added
// in the same order, so the rbar is bit-identical to the one a full last pass would have left.  n_iter == 0: no pass,
// rbar stays the centre.
template <int C>
struct LastPassRbar {
    __device__ __forceinline__ void operator()(const ScanArgs& a, long long o, float Dd, float (&rbar)[C]) const
    {
        if (a.k.n_iter == 0)
            return;
        const VolView& vol = a.vol;
        const int v = (int)(o / vol.U);
        const int u = (int)(o - (long long)v * vol.U);
        const float* epi = vol.row(v, 0);
        const float uf = (float)u;
        const unsigned Um1_bits = __float_as_uint((float)(vol.U - 1));
        const float kq = (C == 1) ? a.k.k1 : a.k.inv_h2;
        const float Ss0 = (float)a.s_hat;
        const int S = vol.S;
        float A[C];
#pragma unroll
        for (int c = 0; c < C; c++)
            A[c] = 0.0f;
        float B = 0.0f;
        constexpr int kBatch = 8;   // loads in flight
#pragma unroll 1
        for (int s0 = 0; s0 < S; s0 += kBatch) {
            float R[C][kBatch];
#pragma unroll
            for (int j = 0; j < kBatch; j++) {
                const int s = min(s0 + j, S - 1);   // (past S: a valid address, the sample is not used)
                float x = (Ss0 - (float)s) * Dd;   // core.hpp:542,550
                x = x * a.k.slope;                 // core.hpp:551
                x = x + uf;                        // core.hpp:552
                const float t = lerp_weight(x);    // interp.hpp:179-181
                const bool ok = __float_as_uint(x) <= Um1_bits;   // interp.hpp:182 (x is never -0)
                const int i0 = ok ? floor_to_int(x) : 0;
                const float* p = epi + (long long)s * vol.stride_s + i0 * C;
                const float omt = 1.0f - t;
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const float m0 = omt * p[c];   // interp.hpp:184
                    const float m1 = t * p[C + c];
                    const float r = m0 + m1;
                    R[c][j] = ok ? r : kSentinel;
                }
            }
#pragma unroll
            for (int j = 0; j < kBatch; j++) {
                if (s0 + j >= S)
                    break;
                float q[C];
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const float delta = R[c][j] - rbar[c];   // core.hpp:591
                    const float tq = kq * delta;             // kernels.cpp:21 / :43
                    q[c] = tq * delta;
                }
                float qs = q[0];
                if (C == 3) {
                    qs = q[0] + q[C - 1];                    // OpenCV 3.x reduceC_: (q0 + q2) + q1
                    qs = qs + q[C > 1 ? 1 : 0];
                }
                const float K = kernel_weight(qs);           // kernels.cpp:23-25 / :51-53
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const float pr = R[c][j] * K;            // core.cpp:28 / :36
                    A[c] = A[c] + pr;                        // core.hpp:602
                }
                B = B + K;                                   // core.hpp:603
            }
        }
#pragma unroll
        for (int c = 0; c < C; c++) {
            const float qd = (B != 0.0f) ? (A[c] / B) : 0.0f;   // core.cpp:42 / :50, OpenCV 3.x: /0 -> 0
            rbar[c] = (qd > 0.0f) ? qd : 0.0f;                  // core.hpp:609
        }
    }
};

// Waves per SIMD the register budget allows: C*SPAD sample registers + ~64 working registers
// (a batch of in-flight samples, the per-pixel state, SGPR overflow lanes), in the hardware's
// 8-register granules, 512 registers per SIMD lane.
constexpr int scan_reg_waves(int spad, int c)
{
    const int regs = ((c * spad + (c == 1 ? 64 : 96) + 7) / 8) * 8;
    const int w = 512 / regs;
    // Measured exceptions (profiles/r01_k2_variants.md): one more wave per SIMD than the budget above allows, the
    // compiler keeping a few dozen sample registers in scratch (coalesced per lane, cheap), wins 4-13 % here ...
    if (c == 1 && spad > 104 && spad <= 144) return 3;
    if (c == 1 && spad >= 80 && spad <= 88) return 4;
    if (c == 3 && spad >= 32 && spad <= 40) return 3;
    // ... and where the working set is smaller than the 64 / 96 assumed, the extra wave costs no scratch at all
    if (c == 1 && (spad == 48 || spad == 40)) return 5;   // 40: c2 (33 views) +2 %
    if (c == 3 && spad == 24) return 4;
    if (c == 1 && spad == 16) return 7;    // c1 (9 views) +2.5 %
    return w > 8 ? 8 : (w < 1 ? 1 : w);
}

// The variants above that run a wave more than their registers allow keep the per-pixel running result in LDS, not in
// registers (BestLds, k2_scan.hpp): nothing is left for hipcc to spill.
#ifndef RSLF_REG_BEST_LDS
#define RSLF_REG_BEST_LDS 1
#endif
constexpr bool scan_reg_best_in_lds(int spad, int c)
{
    if (!RSLF_REG_BEST_LDS)
        return false;
    if (c == 1)
        return spad == 16 || spad == 40 || spad == 48 || (spad >= 80 && spad <= 88) || (spad >= 104 && spad <= 144);
    return spad == 24 || spad == 40;
}

// One wave per SIMD: a wave issues a VALU instruction every ~5 clocks whatever it is (tools/ubench_valu.hip),
// so packed fp32 halves the issue slots of the mean-shift pass.  With two or more waves the SIMD is already
// saturated by scalar instructions and packed ones run at half rate.
constexpr bool scan_reg_packed_math(int spad, int c) { return scan_reg_waves(spad, c) == 1; }

// The row kernels whose scan is TRIM (one channel, scalar math): not the ones that already run a wave per SIMD more than
// their registers allow (scan_reg_waves' measured exceptions, which carry scratch by design): the value the split keeps
// live adds to their spill.  Their last pass stays whole.
constexpr bool scan_reg_trim(int spad, int c)
{
    return c == 1 && !scan_reg_packed_math(spad, c) && spad != 48 && !(spad >= 80 && spad <= 88) && !(spad > 112 && spad <= 144);
}
// The row kernels whose uniform-D scan takes lane-invariant taps from a per-hypothesis table (scan_reg_body, TAPS): the
// 104-slot kernel of the c3 shape, VALU-issue bound at 3 waves per SIMD with registers to spare for neither a wider batch
// nor the table -- its entries live in LDS (+4.9 KiB per workgroup, same occupancy).  Other slot counts stay as they are
// until a same-box A/B shows them a gain (profiles/r10_tap_table.md).
#ifndef RSLF_TAP_TABLE
#define RSLF_TAP_TABLE 1   // 0 builds every row kernel without the table (A/B)
#endif
constexpr bool scan_reg_tap_table(int spad, int c) { return RSLF_TAP_TABLE && c == 1 && spad == 104 && scan_reg_trim(spad, c); }

// The row kernels that also have a SCALAR-TAP form (scan_reg_body_scalar) for hypotheses whose every view offset is
// row-exact (k2_taps.hpp, row_exact_entry): the tap offset and the weights of such an offset are the same for every pixel of
// every scanline, so they come from a per-launch table in memory (ScanArgs::rx_*) by scalar loads and stay in SGPRs.
// The 104-slot kernel only, as the tap table (profiles/r12_scalar_taps.md).
#ifndef RSLF_SCALAR_TAPS
#define RSLF_SCALAR_TAPS 1   // 0 builds the row kernels without the form (A/B): a table handed in is then ignored
#endif
#ifndef RSLF_SCALAR_GB
#define RSLF_SCALAR_GB 13    // loads in flight per gather round of the scalar-tap form: eight rounds per hypothesis at 104 slots
#endif
constexpr bool scan_reg_scalar_taps(int spad, int c) { return RSLF_SCALAR_TAPS && scan_reg_tap_table(spad, c); }

// Uniform-D, interior, TRIM, one channel, and every view offset row-exact: hypotheses [d0, d1) of a tile from the row-exact
// table.  No offset table, no tap_entry, no ballot, no LDS traffic and no division per hypothesis: D[d] and the entries are
// scalar loads, a sample's address is the EPI's scalar base plus the entry's offset (two scalar adds) plus this lane's
// pixel offset (ONE register for the whole kernel), and the blend takes both weights as scalar operands -- the same three
// operations in the same roles as every other form (interp.hpp:184), hence the same bits.  The next round's entries are
// asked for while this round's loads are in flight.  The tile's pixels need not be consecutive.  The gather has no branch
// at all: a padding slot s >= S (only the last kPadSlack slots can be one) repeats the last view's tap with zero weights --
// three loads of lines the round reads anyway at 101 views -- and its register is never read, mean_shift_pass skips it by
// S.  (With the slots' wave-uniform tests the tail of the gather was sixteen small blocks: its loads lost the scalar base
// and the padding selects and SGPR reloads cost 200 VALU per hypothesis, most of what the form saves.)
template <int SPAD, class BestT>
__device__ __forceinline__ void scan_reg_body_scalar(const ScanArgs& a, int v, int u, int d0, int d1, BestT& best)
{
    constexpr int C = 1, BATCH = RSLF_SCALAR_GB, ROUNDS = SPAD / BATCH;
    static_assert(SPAD % BATCH == 0, "whole rounds");
    static_assert(!scan_reg_packed_math(SPAD, 1) && scan_reg_trim(SPAD, 1), "the passes below are the scalar TRIM ones of the other forms");
    // (constant address space: a uniform index is then a scalar load whatever the kernel stores elsewhere)
    typedef const __attribute__((address_space(4))) long long* OffPtr;
    typedef const __attribute__((address_space(4))) f2* WeightPtr;
    typedef const __attribute__((address_space(4))) float* FloatPtr;
    const VolView& vol = a.vol;
    const float* epi = vol.row(v, 0);
    const int S = vol.S;
    const float kq = a.k.k1;                       // kernels.cpp:21
    const unsigned ubytes = (unsigned)u << 2;      // this lane's pixel within the row
    // core.hpp:577: rbar starts from R[s_hat] = E[s_hat][u] for every hypothesis
    const float centre = epi[(long long)a.s_hat * vol.stride_s + u];
    const f2 R2[1][1] = {{f2{0.0f, 0.0f}}};

#pragma unroll 1
    for (int d = d0; d < d1; d++) {
        const float Dd = ((FloatPtr)a.rx_D)[d];
        const OffPtr toff = (OffPtr)a.rx_off + (long long)d * SPAD;
        const WeightPtr tw = (WeightPtr)a.rx_w + (long long)d * SPAD;
        float R[C][SPAD];
        // The offsets of a round are needed before its loads, the weights only once they are back: the weights of this round
        // and the offsets of the next are asked for while the round's loads are in flight.
        long long cur[BATCH], nxt[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; j++)
            cur[j] = toff[j];
#pragma unroll
        for (int g = 0; g < ROUNDS; g++) {
            float e0[BATCH], e1[BATCH];
            f2 w[BATCH];
            // (re-made opaque per round: the zero-extension of the lane's offset then sits beside the loads that add it to their
            // scalar bases, which is what lets them take the base as a scalar operand)
            unsigned ub = ubytes;
            asm volatile("" : "+v"(ub));
            // the round's loads back to back ...
#pragma unroll
            for (int j = 0; j < BATCH; j++) {
                // (the scalar sum is pinned too: left to itself the compiler adds the lane's offset to the EPI's base
                // once and the entry's offset per sample with a 64-bit VALU add)
                typedef const __attribute__((address_space(1))) char* GlobalBytes;
                typedef const __attribute__((address_space(1))) float* GlobalFloats;
                const unsigned long long sum = (unsigned long long)epi + (unsigned long long)cur[j];
                unsigned lo = (unsigned)sum;
                asm volatile("" : "+s"(lo));
                const unsigned long long row = (sum & 0xFFFFFFFF00000000ull) | lo;
                const GlobalFloats p = (GlobalFloats)((GlobalBytes)row + ub);
                e0[j] = p[0];
                e1[j] = p[1];
            }
            // ... this round's weights and the next round's offsets under them ...
#pragma unroll
            for (int j = 0; j < BATCH; j++)
                w[j] = tw[g * BATCH + j];
            if (g + 1 < ROUNDS) {
#pragma unroll
                for (int j = 0; j < BATCH; j++)
                    nxt[j] = toff[(g + 1) * BATCH + j];
            }
            // ... then the blend
#pragma unroll
            for (int j = 0; j < BATCH; j++) {
                const float m0 = w[j].y * e0[j];   // interp.hpp:184: (1 - t) * left tap
                const float m1 = w[j].x * e1[j];
                R[0][g * BATCH + j] = m0 + m1;
            }
            // pin the round (scan_reg_body): no "all loads first, all blends last"
#pragma unroll
            for (int j = 0; j < BATCH; j++)
                asm volatile("" : "+v"(R[0][g * BATCH + j]));
#pragma unroll
            for (int j = 0; j < BATCH; j++)
                cur[j] = nxt[j];
        }

        float rbar[C] = {centre};
        float B = 0.0f;
#pragma unroll 1
        for (int it = 0; it < a.k.n_iter; it++) {   // core.hpp:584-610
            float A[C] = {0.0f};
            B = 0.0f;
            if (it == a.k.n_iter - 1) {
                // the last pass sums K alone, and rbar stays the one that entered it (LastPassRbar)
                mean_shift_pass<SPAD, C, false, true>(R, R2, S, kq, rbar, A, B);
                break;
            }
            mean_shift_pass<SPAD, C, false, false>(R, R2, S, kq, rbar, A, B);
            const float qd = (B != 0.0f) ? (A[0] / B) : 0.0f;   // core.cpp:42, OpenCV 3.x: /0 -> 0
            rbar[0] = (qd > 0.0f) ? qd : 0.0f;                  // core.hpp:609
        }
        const float cardf = (float)S;                  // interior: every sample is inside the row
        float sc = (S != 0) ? (B / cardf) : 0.0f;      // core.hpp:616-620: the last pass's sum of K
        sc = (sc > 0.0f) ? sc : 0.0f;                  // core.hpp:622
        best.offer(sc, d, Dd, rbar);
    }
}

template <int SPAD, int C>
using ScanRegRbarFix = std::conditional_t<scan_reg_trim(SPAD, C), LastPassRbar<C>, NoRbarFix>;

template <int SPAD, int C, class BestT>
__device__ __forceinline__ void scan_reg_rows(const ScanArgs& a, int v, int u, int d0, int d1, BestT& best, float* otab)
{
    constexpr bool PK = scan_reg_packed_math(SPAD, C);
    constexpr bool kTaps = scan_reg_tap_table(SPAD, C);
    if (a.dmin_vu) {
        scan_reg_body<SPAD, C, true, false, PK, 0, BestT, false, scan_reg_trim(SPAD, C)>(a, v, u, d0, d1, best, otab);
        return;
    }
    // the validity test is decided per hypothesis, as in the streaming kernel (scan_stream_rows): runs of hypotheses whose
    // sample lines stay inside the row for every lane take the form without it, in ascending order
    const float max_ds = (float)max(a.s_hat, a.vol.S - 1 - a.s_hat);
    const float range = a.dmax - a.dmin, denom = (float)(a.dim_d - 1);
    const float uf = (float)u, Um1 = (float)(a.vol.U - 1);
    if constexpr (scan_reg_scalar_taps(SPAD, C)) {
        // With the launch's row-exact table (ScanArgs::rx_*) the runs are of (interior, row-exact) hypotheses and D[d] is the
        // table's, so nothing here divides: interior row-exact runs take the scalar-tap form, the others the forms below.
        // Without one (null pointers) the runs and the forms are the ones below.
        typedef const __attribute__((address_space(4))) float* FloatPtr;
        typedef const __attribute__((address_space(4))) int* IntPtr;
        const bool rx = a.rx_off != nullptr;
        auto form = [&](int d) -> int {   // 0 border, 1 interior, 2 interior and row-exact
            const float Dd = rx ? ((FloatPtr)a.rx_D)[d] : hypothesis(a.dmin, range, denom, d);
            const float reach = max_ds * fabsf(Dd) * fabsf(a.k.slope) + 2.0f;
            const bool in = __all((uf - reach >= 0.0f) && (uf + reach <= Um1));
            return !in ? 0 : (rx && ((IntPtr)a.rx_exact)[d]) ? 2 : 1;
        };
        int d = d0;
        while (d < d1) {
            const int f = form(d);
            int e = d + 1;
            while (e < d1 && form(e) == f)
                e++;
            if (f == 2)
                scan_reg_body_scalar<SPAD>(a, v, u, d, e, best);
            else if (f == 1)
                scan_reg_body<SPAD, C, false, true, PK, 0, BestT, false, scan_reg_trim(SPAD, C), kTaps>(a, v, u, d, e, best, otab);
            else
                scan_reg_body<SPAD, C, true, true, PK, 0, BestT, false, scan_reg_trim(SPAD, C)>(a, v, u, d, e, best, otab);
            d = e;
        }
        return;
    }
    auto interior = [&](int d) -> bool {
        const float reach = max_ds * fabsf(hypothesis(a.dmin, range, denom, d)) * fabsf(a.k.slope) + 2.0f;
        return __all((uf - reach >= 0.0f) && (uf + reach <= Um1));
    };
    int d = d0;
    while (d < d1) {
        const bool in = interior(d);
        int e = d + 1;
        while (e < d1 && interior(e) == in)
            e++;
        if (in)
            scan_reg_body<SPAD, C, false, true, PK, 0, BestT, false, scan_reg_trim(SPAD, C), kTaps>(a, v, u, d, e, best, otab);
        else
            scan_reg_body<SPAD, C, true, true, PK, 0, BestT, false, scan_reg_trim(SPAD, C)>(a, v, u, d, e, best, otab);
        d = e;
    }
}

template <int SPAD, int C>
__global__ __launch_bounds__(64 * kScanWaves) __attribute__((amdgpu_waves_per_eu(scan_reg_waves(SPAD, C), scan_reg_waves(SPAD, C))))
void k2_scan_reg(ScanArgs a)
{
    // per wave: the view offsets of a hypothesis; with the tap table (scan_reg_body, TAPS) also the addresses and weight pairs
    __shared__ __attribute__((aligned(16))) float s_otab[kScanWaves][SPAD * (scan_reg_tap_table(SPAD, C) ? 4 : 1)];
    float* otab = s_otab[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
    constexpr bool kEpiDyn = false;
    float* const epi_lds = nullptr;
    const int epi_stride = 0;
    using Fix = ScanRegRbarFix<SPAD, C>;
    if constexpr (scan_reg_best_in_lds(SPAD, C)) {
        __shared__ float s_best[kScanWaves][BestLds<C>::kFloats];
        BestLds<C> running(s_best[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)]);
        RSLF_SCAN_ROW_TILE_FIX((running.init(), scan_reg_rows<SPAD, C>(a, v, u, d0, d1, running, otab), running.load(best)), Fix{})
    } else {
        RSLF_SCAN_ROW_TILE_FIX((scan_reg_rows<SPAD, C>(a, v, u, d0, d1, best, otab)), Fix{})
    }
}

// Packed tiles: its own kernel, because per-lane EPI bases cost address registers the row kernel's
// budget does not have (and must not pay for).
#ifndef RSLF_PACKED_LONG_GB
#define RSLF_PACKED_LONG_GB 4   // divisor: a quarter of the unit per gather batch
#endif
constexpr bool packed_long_unit(int spad, int c) { return c == 1 && spad >= 80 && spad <= 128 && spad % RSLF_PACKED_LONG_GB == 0; }
constexpr int packed_waves(int spad, int c) { return packed_long_unit(spad, c) ? 2 : scan_reg_waves(spad + 24, c); }
constexpr int packed_gather_batch(int spad, int c) { return packed_long_unit(spad, c) ? spad / RSLF_PACKED_LONG_GB : 0; }

template <int SPAD, int C>
__global__ __launch_bounds__(64 * kScanWaves) __attribute__((amdgpu_waves_per_eu(packed_waves(SPAD, C), packed_waves(SPAD, C))))
void k2_scan_reg_packed(ScanArgs a)
{
    // (Tiles whose 64 entries sit on one scanline -- most of them on a visit that scans many pixels -- were also given
    // the row kernel's forms, scalar EPI base and shared offset table: no gain, not kept.)
    constexpr bool kEpiDyn = false;
    float* const epi_lds = nullptr;
    const int epi_stride = 0;
    RSLF_SCAN_PACKED_LOOP((scan_reg_body<SPAD, C, true, false, packed_waves(SPAD, C) == 1, packed_gather_batch(SPAD, C)>(a, v, u, d0, d1, best, nullptr)))
}

// Sparse launches, lanes own HYPOTHESES (k2_scan_reg_px).  A sparse visit's pixels sit two or three to a scanline: with a
// pixel per lane (k2_scan_reg_packed) every load of the gather touches up to 64 scanlines -- 64 cache lines for 512 useful
// bytes -- and the kernel runs at 1.0 G units/s on a list of scattered pixels where the dense kernel makes 8 (c3 shape,
// tools/probe_sparse.py).  Here a wave owns ONE pixel and its lanes score 64 hypotheses of it: a load's 64 taps lie within
// (d_63 - d_0) * |s_hat - s| pixels of one EPI row, a handful of lines, the EPI base is a scalar, and nothing is shared
// between workgroups -- no hypothesis groups, no records, no tickets.  px_waves = 1 / 2 / 4 waves share a pixel's
// hypotheses (lane slot + k * 64 * px_waves; plan::px_waves picks by lane use), so a workgroup holds 4 / 2 / 1 pixels.
// The arithmetic of a (pixel, hypothesis) unit is scan_reg_body's per-lane form, the one per-pixel [dmin, dmax] planes
// take: same operations, same bits.  What changes is the reduction over hypotheses, now across lanes (scan_px_finish,
// k2_scan.hpp).
// Occupancy and gather batch: the ROW kernel's (scalar EPI base, near-coalesced loads: three waves per SIMD and 13 loads in
// flight at 104 slots), not the packed kernel's (two waves, a quarter of the unit in flight): same-box A/B, c3 sweep 118.0
// vs 120.0 ms, SkysatLR-like fine-to-coarse 257 vs 278 ms (profiles/r03_k2_variants.md section 5).  0 builds the other.
#ifndef RSLF_PX_ROWLIKE
#define RSLF_PX_ROWLIKE 1
#endif
constexpr int px_kernel_waves(int spad, int c) { return RSLF_PX_ROWLIKE ? scan_reg_waves(spad, c) : packed_waves(spad, c); }
template <int SPAD, int C>
__global__ __launch_bounds__(64 * kScanWaves) __attribute__((amdgpu_waves_per_eu(px_kernel_waves(SPAD, C), px_kernel_waves(SPAD, C))))
void k2_scan_reg_px(ScanArgs a)
{
    __shared__ double s_sum[kScanWaves];
    __shared__ float s_rec[kScanWaves][kPxRecFloats];
    const int n = *a.packed_n;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wpp = a.px_waves, ppw = kScanWaves / wpp;   // waves per pixel, pixels per workgroup
    const int items = (n + ppw - 1) / ppw;
    const int sub = wave % wpp;
    const int dlane = sub * 64 + lane, dstep = 64 * wpp;
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const int e = item * ppw + wave / wpp;
        const bool listed = e < n;   // (a workgroup's last pixels may be missing: those waves shadow the list's last entry and write nothing)
        const unsigned o = (unsigned)__builtin_amdgcn_readfirstlane(a.list[listed ? e : n - 1]);
        const int v = (int)(o / (unsigned)a.vol.U);
        const int u = (int)(o - (unsigned)v * (unsigned)a.vol.U);
        const bool have = listed && scan_px_owns(a, v);   // (wave-uniform; a row with many pixels is the row-tile launch's)
        Best<C> best;
        best.init();
        // the validity test (interp.hpp:182) can go where every sample line of every hypothesis stays inside the row
        const float dlo = a.dmin_vu ? a.dmin_vu[o] : a.dmin, dhi = a.dmax_vu ? a.dmax_vu[o] : a.dmax;
        const float reach = (float)max(a.s_hat, a.vol.S - 1 - a.s_hat) * fmaxf(fabsf(dlo), fabsf(dhi)) * fabsf(a.k.slope) + 2.0f;
        const bool interior = (float)u - reach >= 0.0f && (float)u + reach <= (float)(a.vol.U - 1);   // wave-uniform
        constexpr int kGB = RSLF_PX_ROWLIKE ? 0 : packed_gather_batch(SPAD, C);
        if (!have) {
            // nothing to scan: the finish below still runs (its barriers are the workgroup's)
        } else if (interior)
            scan_reg_body<SPAD, C, false, false, false, kGB, Best<C>, true>(a, v, u, 0, a.dim_d, best, nullptr, dlane, dstep);
        else
            scan_reg_body<SPAD, C, true, false, false, kGB, Best<C>, true>(a, v, u, 0, a.dim_d, best, nullptr, dlane, dstep);
        scan_px_finish<C>(a, o, have, best, wave, lane, wpp, s_rec, s_sum);   // across the lanes, then the waves that share the pixel
    }
}

}  // namespace rslf
