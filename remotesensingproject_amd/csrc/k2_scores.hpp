// K2, score rows (k2_score_rows_reg / k2_score_rows_generic): the scan with every hypothesis' score kept.
//
// compute_1D_depth_epi writes score[d] of each pixel into row u of the caller's buf_scores_u_d (core.hpp:616-625) before it
// takes the arg max (:634) and C_d (:641) from that row.  These kernels are the scan kernels (k2_reg.hpp, k2_scan.hpp) with
// another sink behind offer(): instead of a running best, the scores go to [row of the window][u][d], d fastest.  Same work
// mapping -- 64 list entries of one scanline per workgroup, its four waves a quarter of the hypotheses each, lane = pixel --
// same arithmetic, so the same bits as the score the scan keeps for its winner.  No epilogue: nothing is merged, every
// (tile, group) workgroup writes its own slice.
#pragma once

#include "k2_reg.hpp"
#include "rslf_plan.hpp"

namespace rslf {

constexpr int kScoreRun = plan::kScoreRun;
constexpr int kScorePitch = kScoreRun + 1;   // floats per pixel of a wave's parking block
static_assert(64 % kScoreRun == 0, "a store instruction covers whole runs");

// Where the rows go (the sink's own pointers: ScanArgs stays the scan's)
struct ScoreDst {
    float* scores;   // [n_rows][U][dim_d]
    int v_first;     // the window's first scanline
};

// The sink.  offer() is reached once per hypothesis, wave-uniformly, in ascending d from the wave's d_lo: the lane parks its
// score at [pixel = lane][d - start of the run].  One dword per lane straight to memory would put every lane on a cache
// line of its own (pixels are dim_d floats apart); so after kScoreRun hypotheses, or the wave's last one, the block goes out
// TRANSPOSED: per store instruction 64 / kScoreRun pixels x kScoreRun consecutive d, i.e. runs of 64 contiguous bytes.
// LDS within a wave is in order, so parking stores and transposed reads need no more than the compiler's respect.
// Lanes that hold no pixel of their own (scan_tile makes them shadow the tile's last one) have pixel number -1: never written.
template <int C>
struct ScoreRows {
    float* park;      // this wave's block, kScorePitch floats per lane
    const int* pix;   // this wave's pixel numbers u per lane, -1 = none
    float* row;       // scores of pixel 0 of this scanline
    int dim_d, d_lo, d_hi;
    __device__ __forceinline__ ScoreRows(float* park_, int* pix_, const ScanArgs& a, const ScoreDst& dst, int v, int u, bool active,
                                         int d0, int d1)
        : park(park_), pix(pix_), row(dst.scores + (size_t)(v - dst.v_first) * (size_t)a.vol.U * (size_t)a.dim_d), dim_d(a.dim_d),
          d_lo(d0), d_hi(d1)
    {
        pix_[threadIdx.x & 63] = active ? u : -1;
    }
    __device__ __forceinline__ void offer(float sc, int d, float, const float (&)[C])
    {
        const int k = (d - d_lo) % kScoreRun;   // (wave-uniform)
        park[(threadIdx.x & 63) * kScorePitch + k] = sc;
        if (k == kScoreRun - 1 || d == d_hi - 1)
            flush(d - k, k + 1);
    }
    __device__ __forceinline__ void flush(int d_first, int n)
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int lane = threadIdx.x & 63;
        const int j = lane % kScoreRun, q = lane / kScoreRun;
#pragma unroll 4
        for (int p0 = 0; p0 < 64; p0 += 64 / kScoreRun) {
            const int p = p0 + q;
            const float sc = park[p * kScorePitch + j];
            const int u = pix[p];
            if (j < n && u >= 0)
                row[(size_t)u * (size_t)dim_d + (size_t)(d_first + j)] = sc;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
};

// The row kernels' last pass sums K alone wherever scan_reg_body can (one channel, scalar math): the score needs nothing
// else, and no rbar is kept here.  Elsewhere the whole last pass runs.
constexpr bool score_rows_trim(int spad, int c) { return c == 1 && !scan_reg_packed_math(spad, c); }
constexpr bool score_rows_tap_table(int spad, int c) { return scan_reg_tap_table(spad, c) && score_rows_trim(spad, c); }

// scan_reg_rows (k2_reg.hpp) for this sink: per-pixel ranges take the per-lane form; else runs of hypotheses whose sample
// lines stay inside the row for every lane take the form without the validity test, in ascending order.
template <int SPAD, int C>
__device__ __forceinline__ void score_reg_rows(const ScanArgs& a, int v, int u, int d0, int d1, ScoreRows<C>& rows, float* otab)
{
    constexpr bool PK = scan_reg_packed_math(SPAD, C);
    constexpr bool kTrim = score_rows_trim(SPAD, C);
    constexpr bool kTaps = score_rows_tap_table(SPAD, C);
    if (a.dmin_vu) {
        scan_reg_body<SPAD, C, true, false, PK, 0, ScoreRows<C>, false, kTrim>(a, v, u, d0, d1, rows, otab);
        return;
    }
    const float max_ds = (float)max(a.s_hat, a.vol.S - 1 - a.s_hat);
    const float range = a.dmax - a.dmin, denom = (float)(a.dim_d - 1);
    const float uf = (float)u, Um1 = (float)(a.vol.U - 1);
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
            scan_reg_body<SPAD, C, false, true, PK, 0, ScoreRows<C>, false, kTrim, kTaps>(a, v, u, d, e, rows, otab);
        else
            scan_reg_body<SPAD, C, true, true, PK, 0, ScoreRows<C>, false, kTrim>(a, v, u, d, e, rows, otab);
        d = e;
    }
}

// One (tile, group) item of a row-tile launch: which scanline, which pixel per lane, which hypotheses for this wave.
#define RSLF_SCORE_ROW_TILE(SCAN_CALL)                                                                                     \
    __shared__ float s_park[kScanWaves][64 * kScorePitch];                                                                 \
    __shared__ int s_pix[kScanWaves][64];                                                                                  \
    int v, u, d0, d1;                                                                                                      \
    bool active;                                                                                                           \
    const int lb = RSLF_XCD_ROW_INTERLEAVE ? xcd_logical_block_rows(blockIdx.x, a.tiles_per_row * a.groups)                \
                                           : xcd_logical_block(blockIdx.x, a.per_xcd);                                     \
    if (!scan_tile(a, lb, v, u, active))                                                                                   \
        return;                                                                                                            \
    scan_chunk(a, lb % a.groups, d0, d1);                                                                                  \
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                                                     \
    ScoreRows<C> rows(s_park[wave], s_pix[wave], a, dst, v, u, active, d0, d1);                                            \
    SCAN_CALL;

template <int SPAD, int C>
__global__ __launch_bounds__(64 * kScanWaves) __attribute__((amdgpu_waves_per_eu(scan_reg_waves(SPAD, C), scan_reg_waves(SPAD, C))))
void k2_score_rows_reg(ScanArgs a, ScoreDst dst)
{
    constexpr int kTable = score_rows_tap_table(SPAD, C) ? 4 : 1;
    __shared__ __attribute__((aligned(16))) float s_otab[kScanWaves][SPAD * kTable];
    static_assert(sizeof(float) * kScanWaves * (64 * kScorePitch + 64 + SPAD * kTable) == plan::score_lds_bytes(SPAD, kTable) &&
                      plan::score_lds_bytes(SPAD, kTable) <= plan::kScoreLdsLimit, "rslf_plan.hpp states this kernel's LDS");
    float* otab = s_otab[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
    RSLF_SCORE_ROW_TILE((score_reg_rows<SPAD, C>(a, v, u, d0, d1, rows, otab)))
}

// Everything else -- view counts beyond the register kernels' slots, radiances out of their range, the nearest-neighbour
// modes, "force_scan" -- with the generic arithmetic, one hypothesis at a time through scan_generic_body's running best:
// after one hypothesis that is its score.
template <int C>
__global__ __launch_bounds__(64 * kScanWaves) void k2_score_rows_generic(ScanArgs a, ScoreDst dst)
{
    RSLF_SCORE_ROW_TILE(for (int d = d0; d < d1; d++) {
        Best<C> one;
        one.init();
        scan_generic_body<C>(a, v, u, d, d + 1, one);
        rows.offer(one.score, d, one.D, one.rbar);
    })
}

// The window's pixel lists: ascending u of the pixels of scanline v_first + blockIdx.x whose mask byte is set (every pixel
// without a mask), as the scan kernels' row tiles read them (scan_tile: list[v * U + i], count[v]).  The mask is not written.
__global__ __launch_bounds__(256) void k_score_lists(const uint8_t* __restrict__ mask, int U, int v_first, int* __restrict__ list,
                                                     int* __restrict__ count, unsigned long long* __restrict__ total)
{
    const int v = v_first + blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __shared__ int wave_tot[4];
    __shared__ int base_s;
    if (threadIdx.x == 0)
        base_s = 0;
    __syncthreads();
    for (int u0 = 0; u0 < U; u0 += 256) {
        const int u = u0 + threadIdx.x;
        const bool f = u < U && (!mask || mask[(long long)v * U + u] != 0);
        const unsigned long long b = __ballot(f);
        const int rank = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0)
            wave_tot[w] = __popcll(b);
        __syncthreads();
        int off = base_s;
        for (int i = 0; i < w; i++)
            off += wave_tot[i];
        if (f)
            list[(long long)v * U + off + rank] = u;
        __syncthreads();
        if (threadIdx.x == 0)
            base_s += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        count[v] = base_s;
        atomicAdd(total, (unsigned long long)base_s);
    }
}

}  // namespace rslf
