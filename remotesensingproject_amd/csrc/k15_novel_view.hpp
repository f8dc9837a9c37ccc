// K15: the novel view (rslf_novel_view).  Not in the reference: K14 (k14_view_warp.hpp) with its second half -- every target
// pixel gets a disparity (cracks and disocclusions filled from the background side), and its colour is gathered backwards
// along that disparity from the views that see the point, blended at sub-pixel positions.  The per-pixel rule is
// k15_novel_rule.hpp, the one statement the host tests compile too; this file is how the device walks it.
//
// One workgroup of 256 threads per (target, scanline), K14's grid (xcd_logical_block_rows: a scanline's S rows serve all its
// targets from one L2), up to 256 targets in the arguments, no scratch.
//
// A. K14's scatter, restated (sharing the loop would put a template parameter into K14's kernel): one 64-bit key per column
//    in dynamic LDS, an atomicMax per candidate.  After the barrier each thread decodes a CONTIGUOUS chunk of columns
//    (plan::novel_chunk: 32 at the cap) and writes {disparity bits, hit} back into the same 8 bytes: no second array.
// B. The fill is a segmented scan -- "last hit at or before", "first hit at or after": a thread's chunk gives two partials
//    (novel_chunk_partials), wave shuffles and 32 bytes of LDS carry them across the 256 threads, and a second pass over the
//    chunk writes the filled columns' entries (novel_chunk_fill).  Bounds are hit columns, which nobody rewrites, so a thread
//    may read them in another thread's chunk after the barrier.
// C. Four adjacent columns per thread, the quads strided by the block, so a wave's gathers fall on neighbouring columns and
//    the planes leave in 16-byte stores.  The views are walked in rank order; the loads of a view -- disparity, validity byte
//    and the 2 * C taps of each of the four pixels -- are issued UNCONDITIONALLY at clamped columns before the first test
//    (k4_propagate.hpp and profiles/r19_consistency.md record what a load under `if` costs with this compiler).  A wave
//    leaves the walk when a vote says that every lane has its `sources`.  CT: the volume's channels, 1 or 3 (what a volume can
//    have: rslf_volume_create); -1: no volume (n_src and row_cov alone).
//
// Every index into LDS and every conversion to int sits behind the rule's guards (warp_candidate, warp_source_column,
// novel_tap): no input value -- NaN, +-inf, 1e30, a huge slope -- reaches an address.
#pragma once

#include "k15_novel_rule.hpp"
#include "rslf_device.hpp"
#include "rslf_plan_novel.hpp"

namespace rslf {

struct NovelArgs {
    const float* depth;     // [S][V][U]
    const uint8_t* valid;   // [S][V][U], nullable
    int S, V, U;
    float slope;
    int radius, nearer, max_gap, sources;
    float tol;
    int T;                  // the targets of THIS launch
    int k_first;            // ... whose planes start at target k_first of the call's
    int vec;                // 16-byte stores: U is a multiple of four and every plane asked for is 16-byte aligned
    VolView vol;            // base NULL: no volume
    float* colour;          // [T][V][U][C]
    float* out_depth;       // [T][V][U] each, nullable
    uint8_t* fill;
    int32_t* n_src;
    float* err;
    double* row_err;        // [T][V]
    int32_t* row_cov;
    float target[plan::kWarpLaunchTargets];
    int32_t exclude[plan::kWarpLaunchTargets];
};

template <typename T4, typename T>
__device__ __forceinline__ void novel_store4(T* plane, long long o, const T (&x)[4], int n, bool vec)
{
    if (!plane)
        return;
    if (vec) {
        T4 q;
        q.x = x[0], q.y = x[1], q.z = x[2], q.w = x[3];
        *reinterpret_cast<T4*>(plane + o) = q;
    } else {
        for (int j = 0; j < n; j++)
            plane[o + j] = x[j];
    }
}

// HAS_VALID = false: a.valid is NULL and never read.
template <bool HAS_VALID, int CT>
__global__ __launch_bounds__(plan::kWarpBlock) void k15_novel_view(NovelArgs a)
{
    constexpr int B = plan::kWarpBatch, W = plan::kWarpBlock, NW = W / kWave;
    constexpr bool VOL = CT >= 0;
    constexpr int CC = CT > 0 ? CT : 1, C = VOL ? CT : 0;
    constexpr int C1 = CC > 1 ? 1 : 0, C2 = CC > 2 ? 2 : 0;
    extern __shared__ unsigned long long s_novel[];   // [U]: keys, then entries
    __shared__ int s_last[NW], s_first[NW];
    __shared__ double s_row_err[NW];
    __shared__ int s_row_cov[NW];
    const int lb = xcd_logical_block_rows((int)blockIdx.x, a.T);
    const int v = lb / a.T;
    if (v >= a.V)
        return;   // the surplus blocks of a launch rounded up to eight scanlines
    const int k = lb - v * a.T;
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const float t = a.target[k];
    const int exclude = a.exclude[k];
    const int U = a.U;
    const long long plane = (long long)a.V * U, row = (long long)v * U;

    // ---- A: the z-buffer (k14_view_warp.hpp's loop) ----
    for (int u = tid; u < U; u += W)
        s_novel[u] = 0ull;
    __syncthreads();
    {
        WarpWalk walk = warp_walk_start(t, a.S);   // workgroup-uniform
        int s = 0, rank = 0;
        while (warp_walk_next(&walk, t, a.S, &s)) {
            const int r = rank++;
            if (!warp_in_window(s, t, a.radius))
                break;   // the walk leaves t: every later view is farther
            if (s == exclude)
                continue;
            const float* const drow = a.depth + (long long)s * plane + row;
            const uint8_t* const vrow = HAS_VALID ? a.valid + (long long)s * plane + row : nullptr;
            for (int u0 = 0; u0 < U; u0 += W * B) {
                float d[B];
                uint8_t vb[B];
#pragma unroll
                for (int j = 0; j < B; j++) {
                    const int u = u0 + j * W + tid;
                    const int uc = u < U ? u : U - 1;
                    d[j] = drow[uc];
                    vb[j] = HAS_VALID ? vrow[uc] : (uint8_t)255;
                }
#pragma unroll
                for (int j = 0; j < B; j++) {
                    const int u = u0 + j * W + tid;
                    int x = 0;
                    if (u < U && warp_candidate(d[j], vb[j], s, u, U, t, exclude, a.radius, a.slope, &x))   // x in [0, U)
                        atomicMax(&s_novel[x], warp_key(warp_z(d[j], a.nearer), r, s));
                }
            }
        }
    }
    __syncthreads();

    // ---- decode a contiguous chunk in place, and its two partials ----
    const int chunk = (U + W - 1) / W;
    const int x0 = tid * chunk < U ? tid * chunk : U, x1 = x0 + chunk < U ? x0 + chunk : U;
    for (int x = x0; x < x1; x++) {
        const unsigned long long key = s_novel[x];
        if (key) {
            int sv = warp_key_view(key);
            sv = sv < a.S ? sv : a.S - 1;
            const int su = warp_source_column(key, x, U, t, a.nearer, a.slope);
            s_novel[x] = novel_entry(kNovelHit, warp_float_bits(a.depth[(long long)sv * plane + row + su]));   // the winner's own bits
        }
    }
    int last, first;
    novel_chunk_partials(s_novel, x0, x1, U, &last, &first);

    // ---- B: the scan over the threads, then the second pass ----
    int incl = last, sfx = first;
    for (int o = 1; o < kWave; o <<= 1) {
        const int up = __shfl_up(incl, o), down = __shfl_down(sfx, o);
        incl = lane >= o && up > incl ? up : incl;
        sfx = lane + o < kWave && down < sfx ? down : sfx;
    }
    int before = __shfl_up(incl, 1), after = __shfl_down(sfx, 1);
    before = lane == 0 ? -1 : before;
    after = lane == kWave - 1 ? U : after;
    if (lane == kWave - 1)
        s_last[wave] = incl;
    if (lane == 0)
        s_first[wave] = sfx;
    __syncthreads();
    for (int w = 0; w < NW; w++) {
        before = w < wave && s_last[w] > before ? s_last[w] : before;
        after = w > wave && s_first[w] < after ? s_first[w] : after;
    }
    novel_chunk_fill(s_novel, x0, x1, U, before, after, a.max_gap, a.nearer);
    __syncthreads();

    // ---- C: gather and blend, four adjacent columns per thread ----
    const bool gather = VOL || a.n_src || a.row_cov || a.row_err;   // workgroup-uniform
    int tv = (int)t;   // |t| <= 65536; the slab's own row, read only for err (t is then a view)
    tv = tv < 0 ? 0 : tv >= a.S ? a.S - 1 : tv;
    const bool want_err = VOL && (a.err || a.row_err);
    const float* const lrow = want_err ? a.vol.row(v, tv) : nullptr;
    const long long out_row = ((long long)(a.k_first + k) * a.V + v) * U;
    const bool vec = a.vec != 0;
    double esum = 0.0;
    int ncov = 0;
    for (int q = tid; 4 * q < U; q += W) {
        const int n = U - 4 * q < 4 ? U - 4 * q : 4;
        const long long o = out_row + 4 * q;
        uint8_t code[4];
        float d[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const unsigned long long e = j < n ? s_novel[4 * q + j] : 0ull;
            code[j] = (uint8_t)novel_entry_code(e);
            d[j] = code[j] ? novel_entry_depth(e) : 0.0f;
        }
        if (a.fill) {
            if (vec)
                *reinterpret_cast<uint32_t*>(a.fill + o) = (uint32_t)code[0] | (uint32_t)code[1] << 8 | (uint32_t)code[2] << 16 | (uint32_t)code[3] << 24;
            else
                for (int j = 0; j < n; j++)
                    a.fill[o + j] = code[j];
        }
        novel_store4<float4>(a.out_depth, o, d, n, vec);
        if (!gather)
            continue;

        int32_t nsrc[4] = {0, 0, 0, 0};
        float eacc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, wsum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool seen[4] = {false, false, false, false};   // a view of the walk was in field
        {
            float acc[4][CC], fst[4][CC];   // the blend, and the first view in field (then: the colour)
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int c = 0; c < CC; c++)
                    acc[j][c] = fst[j][c] = 0.0f;
            WarpWalk walk = warp_walk_start(t, a.S);
            int s = 0;
            while (warp_walk_next(&walk, t, a.S, &s)) {
                if (!warp_in_window(s, t, a.radius))
                    break;
                if (s == exclude)
                    continue;
                const float* const drow = a.depth + (long long)s * plane + row;
                const uint8_t* const vrow = HAS_VALID ? a.valid + (long long)s * plane + row : nullptr;
                const float* const erow = VOL ? a.vol.row(v, s) : nullptr;
                NovelTap tap[4];
                float dt[4], e0[4][CC], e1[4][CC];
                uint8_t vb[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {   // every index is in [0, U) whatever d holds
                    tap[j] = novel_tap(d[j], s, 4 * q + j, U, t, a.slope);
                    dt[j] = drow[tap[j].ur];
                    vb[j] = HAS_VALID ? vrow[tap[j].ur] : (uint8_t)255;
                    if (VOL) {
#pragma unroll
                        for (int c = 0; c < CC; c++) {
                            e0[j][c] = erow[(long long)tap[j].i0 * C + c];
                            e1[j][c] = erow[(long long)tap[j].i1 * C + c];
                        }
                    }
                }
                const float g = novel_weight(s, t);
                bool done = true;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const bool live = (code[j] != 0) & (nsrc[j] < a.sources) & tap[j].in_field;
                    const bool agrees = live & novel_agrees(dt[j], vb[j], d[j], a.tol);
                    if (VOL) {
#pragma unroll
                        for (int c = 0; c < CC; c++) {
                            const float sample = novel_lerp(tap[j].w, e0[j][c], e1[j][c]);
                            const float gs = g * sample;
                            fst[j][c] = live & !seen[j] ? sample : fst[j][c];
                            acc[j][c] = agrees ? acc[j][c] + gs : acc[j][c];
                        }
                    }
                    seen[j] = seen[j] | live;
                    wsum[j] = agrees ? wsum[j] + g : wsum[j];
                    nsrc[j] += agrees ? 1 : 0;
                    done = done & ((code[j] == 0) | (nsrc[j] >= a.sources));
                }
                if (__all(done))
                    break;   // wave-uniform: every lane of the wave has its sources
            }
            if (VOL) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int x = 4 * q + j < U ? 4 * q + j : U - 1;
#pragma unroll
                    for (int c = 0; c < CC; c++) {
                        const float col = nsrc[j] > 0 ? acc[j][c] / wsum[j] : fst[j][c];
                        fst[j][c] = col;
                        if (want_err)
                            eacc[j] = eacc[j] + fabsf(col - lrow[(long long)x * C + c]);
                    }
                }
                if (a.colour) {
                    if (CT == 1) {
                        const float cq[4] = {fst[0][0], fst[1][0], fst[2][0], fst[3][0]};
                        novel_store4<float4>(a.colour, o, cq, n, vec);
                    } else if (CT == 3 && vec) {   // twelve floats from a 16-byte boundary: (out_row + 4 q) * 3 is a multiple of four
                        float4* const dst = reinterpret_cast<float4*>(a.colour + o * 3);
                        dst[0] = make_float4(fst[0][0], fst[0][C1], fst[0][C2], fst[1][0]);
                        dst[1] = make_float4(fst[1][C1], fst[1][C2], fst[2][0], fst[2][C1]);
                        dst[2] = make_float4(fst[2][C2], fst[3][0], fst[3][C1], fst[3][C2]);
                    } else {
                        for (int j = 0; j < n; j++)
#pragma unroll
                            for (int c = 0; c < CC; c++)
                                a.colour[(o + j) * C + c] = fst[j][c];
                    }
                }
            }
        }
        float ee[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool taken = (nsrc[j] > 0) | seen[j];
            ee[j] = want_err && taken ? eacc[j] / (float)C : 0.0f;
            if (j < n && nsrc[j] > 0) {
                esum += (double)ee[j];
                ncov++;
            }
        }
        novel_store4<int4>(a.n_src, o, nsrc, n, vec);
        if (VOL)
            novel_store4<float4>(a.err, o, ee, n, vec);
    }
    if (a.row_err || a.row_cov) {   // workgroup-uniform
        for (int o = kWave / 2; o > 0; o >>= 1) {
            esum += __shfl_xor(esum, o);
            ncov += __shfl_xor(ncov, o);
        }
        if (lane == 0) {
            s_row_err[wave] = esum;
            s_row_cov[wave] = ncov;
        }
        __syncthreads();
        if (tid == 0) {
            const long long o = (long long)(a.k_first + k) * a.V + v;
            if (a.row_err)
                a.row_err[o] = (s_row_err[0] + s_row_err[1]) + (s_row_err[2] + s_row_err[3]);
            if (a.row_cov)
                a.row_cov[o] = (s_row_cov[0] + s_row_cov[1]) + (s_row_cov[2] + s_row_cov[3]);
        }
    }
}

}  // namespace rslf
