// K6, the renderers: what the reference's getters do between run() and imshow (rslf_plot.cpp:41-110,
// rslf_depth_computation.hpp:374-416, :568-643, :808-891, rslf_fine_to_coarse.hpp:325-378, :432-519).
// Included by rslf_render.hip only (the non-template kernels: one definition per library).
//
//   fit      the two numbers an ImageConverter_uchar holds: min / max, double sums for mean / std, or two order statistics
//            by an exact radix select over order-preserving keys (integer counts: the result does not depend on the
//            order in which workgroups arrive)
//            -- for a whole stack of planes in the same launches: the plane is blockIdx.y, every plane has its own state
//   planes   level -> table -> mask -> shadow cut for a stack of planes in one launch, four adjacent pixels per lane,
//            through one range for all planes or one per plane
//   lines    the z-buffered EPI lines of get_coloured_epi, one workgroup per (scanline, view) row
//
// All three are bandwidth-bound; none uses a float atomic.  Float formulas are single IEEE operations in the reference's
// order (__fmul_rn / __fadd_rn / __fsub_rn: never contracted).
#pragma once

#include "rslf_device.hpp"
#include "rslf_plan.hpp"
#include "rslf_plan_render.hpp"

namespace rslf {

// A plane of rows x cols floats, `row_stride` elements between rows (row v of an [S][V][U] stack is an S x U plane), and
// its validity bytes with the same strides (nullable): a pixel whose byte is 0 counts as 0.0f.  In a batch plane k
// starts `plane_stride` elements after plane k - 1.
struct PlaneView {
    const float* p;
    const uint8_t* valid;
    int rows, cols;
    long long row_stride, plane_stride;
    int vec;   // cols and both strides multiples of 4, p 16-byte and valid 4-byte aligned: a quad is one 16-byte load
};

__device__ __forceinline__ PlaneView plane_of(PlaneView pv, int k)   // plane k of the batch
{
    pv.p += (long long)k * pv.plane_stride;
    if (pv.valid)
        pv.valid += (long long)k * pv.plane_stride;
    return pv;
}

// Pixels 4q .. 4q + 3 of the plane's row-major order (n = rows * cols of them); returns how many exist.
__device__ __forceinline__ int load_quad(const PlaneView& pv, int q, int n, float (&x)[4])
{
    const int i0 = 4 * q;
    if (pv.vec) {
        const int r = i0 / pv.cols, c = i0 - r * pv.cols;
        const long long o = (long long)r * pv.row_stride + c;
        const float4 f = *reinterpret_cast<const float4*>(pv.p + o);
        x[0] = f.x, x[1] = f.y, x[2] = f.z, x[3] = f.w;
        if (pv.valid) {
            const uint32_t m = *reinterpret_cast<const uint32_t*>(pv.valid + o);
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (!((m >> (8 * j)) & 255u))
                    x[j] = 0.0f;
        }
        return 4;
    }
    const int cnt = min(4, n - i0);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        x[j] = 0.0f;
        if (j < cnt) {
            const int r = (i0 + j) / pv.cols, c = (i0 + j) - r * pv.cols;
            const long long o = (long long)r * pv.row_stride + c;
            x[j] = (pv.valid && !pv.valid[o]) ? 0.0f : pv.p[o];
        }
    }
    return cnt;
}

// ---- fit: min / max / double sums -----------------------------------------------------------------------------------
// cv::minMaxLoc and cv::meanStdDev's sums (rslf_plot.cpp:52-53, :88-91).  Every thread sums its pixels in double in a
// fixed order, the workgroup adds its threads in a fixed tree, and k6_fit_reduce adds the partials of the slab in a
// fixed order: the same bits on every run (no atomics).  The unit of that order is the SUM BLOCK: a plane of n pixels
// has `blocks` = plan::fit_blocks(n) of them, whatever the launch; the workgroups of plane blockIdx.y (gridDim.x of
// them, plan::fit_batch_groups) share its sum blocks, so a plane's sums do not depend on the batch it is fitted in.
struct FitPartial {
    double sum, sumsq;
    float mn, mx;
};

__device__ __forceinline__ void fit_combine(FitPartial& a, const FitPartial& b)
{
    a.sum += b.sum;
    a.sumsq += b.sumsq;
    a.mn = fminf(a.mn, b.mn);
    a.mx = fmaxf(a.mx, b.mx);
}

__device__ __forceinline__ void fit_block_reduce(FitPartial acc, FitPartial* __restrict__ dst)
{
    __shared__ FitPartial sh[plan::kFitBlock];
    const int t = threadIdx.x;
    sh[t] = acc;
    __syncthreads();
    for (int o = plan::kFitBlock / 2; o > 0; o >>= 1) {
        if (t < o) {
            FitPartial a = sh[t];
            fit_combine(a, sh[t + o]);
            sh[t] = a;
        }
        __syncthreads();
    }
    if (t == 0)
        *dst = sh[0];
}

__global__ __launch_bounds__(plan::kFitBlock) void k6_fit_stats(PlaneView batch, int n, int blocks, FitPartial* __restrict__ slab)
{
    const PlaneView pv = plane_of(batch, blockIdx.y);
    const int quads = (n + 3) / 4;
    for (int b = blockIdx.x; b < blocks; b += gridDim.x) {   // the same for the whole workgroup
        FitPartial acc{0.0, 0.0, INFINITY, -INFINITY};
        for (int q = b * plan::kFitBlock + threadIdx.x; q < quads; q += blocks * plan::kFitBlock) {
            float x[4];
            const int cnt = load_quad(pv, q, n, x);
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (j < cnt) {
                    const double d = (double)x[j];
                    acc.sum += d;
                    acc.sumsq += d * d;
                    acc.mn = fminf(acc.mn, x[j]);
                    acc.mx = fmaxf(acc.mx, x[j]);
                }
        }
        fit_block_reduce(acc, slab + (long long)blockIdx.y * blocks + b);
        __syncthreads();   // the tree's LDS is free again
    }
}

// One workgroup per plane: slab [plane][blocks] -> out [plane]
__global__ __launch_bounds__(plan::kFitBlock) void k6_fit_reduce(const FitPartial* __restrict__ slab, int blocks, FitPartial* __restrict__ out)
{
    const FitPartial* mine = slab + (long long)blockIdx.x * blocks;
    FitPartial acc{0.0, 0.0, INFINITY, -INFINITY};
    for (int i = threadIdx.x; i < blocks; i += plan::kFitBlock)
        fit_combine(acc, mine[i]);
    fit_block_reduce(acc, out + blockIdx.x);
}

// ---- fit: two order statistics by radix select ------------------------------------------------------------------------
// ImageConverter_uchar::fit(img, true) sorts the plane for two of its elements (rslf_plot.cpp:70-84).  Here: the keys
// (plan::radix_key) are narrowed one 8-bit digit per pass, most significant first, for BOTH ranks in the same passes --
// k6_select_count counts, per rank, the digits of the keys that share the prefix found so far (per-workgroup histograms
// in LDS, merged with one integer atomic per non-empty bin), k6_select_narrow picks each rank's bin
// (plan::radix_bin_holds), extends its prefix, and zeroes the histograms for the next pass.  After plan::kRadixPasses
// passes the prefixes are the keys.  While both ranks share a prefix one histogram serves both.
// A batch keeps one state per plane (st[plane]); k6_select_count has the plane on blockIdx.y, the two one-workgroup
// kernels run one workgroup per plane.  The keys come out as out[plane][2].
struct SelectState {
    uint32_t hist[2][plan::kRadixBins];
    uint32_t prefix[2];
    uint32_t rank[2];
};
static_assert(sizeof(SelectState) == plan::kSelectStateBytes && sizeof(FitPartial) == plan::kFitPartialBytes, "rslf_plan_render.hpp sizes the scratch");

__global__ __launch_bounds__(plan::kRadixBins) void k6_select_init(SelectState* st, uint32_t rank_lo, uint32_t rank_hi)
{
    const int t = threadIdx.x;
    st += blockIdx.x;
    st->hist[0][t] = 0;
    st->hist[1][t] = 0;
    if (t < 2) {
        st->prefix[t] = 0;
        st->rank[t] = t ? rank_hi : rank_lo;
    }
}

// One count per lane with `on`, into an LDS histogram.  A disparity plane holds few distinct values and many exact
// zeros, so most lanes of a wave want the same bin: the digit of the first lane that still has one is counted once for
// every lane that shares it, twice over; only what is left after that goes one atomic per lane.  Call wave-converged.
__device__ __forceinline__ void hist_add(uint32_t* h, bool on, uint32_t d)
{
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int round = 0; round < 2; round++) {
        const unsigned long long m = __ballot(on);
        if (!m)
            return;
        const int lead = __ffsll((long long)m) - 1;
        const uint32_t dl = (uint32_t)__shfl((int)d, lead);
        const unsigned long long eq = __ballot(on && d == dl);
        if (lane == lead)
            atomicAdd(&h[dl], (uint32_t)__popcll(eq));
        on = on && d != dl;
    }
    if (on)
        atomicAdd(&h[d], 1u);
}

__global__ __launch_bounds__(plan::kFitBlock) void k6_select_count(PlaneView batch, int n, int pass, SelectState* st)
{
    __shared__ uint32_t h[2][plan::kRadixBins];
    const int t = threadIdx.x;
    const PlaneView pv = plane_of(batch, blockIdx.y);
    st += blockIdx.y;
    static_assert(plan::kFitBlock == plan::kRadixBins, "one thread per bin");
    h[0][t] = 0;
    h[1][t] = 0;
    const uint32_t p0 = st->prefix[0], p1 = st->prefix[1];
    const bool same = p0 == p1;
    __syncthreads();
    const int quads = (n + 3) / 4;
    for (int q0 = blockIdx.x * plan::kFitBlock; q0 < quads; q0 += gridDim.x * plan::kFitBlock) {   // q0: the same for the whole workgroup
        const int q = q0 + t;
        float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const int cnt = q < quads ? load_quad(pv, q, n, x) : 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t key = plan::radix_key(__float_as_uint(x[j]));
            const uint32_t pre = plan::radix_prefix(key, pass), d = plan::radix_digit(key, pass);
            hist_add(h[0], j < cnt && pre == p0, d);
            if (!same)
                hist_add(h[1], j < cnt && pre == p1, d);
        }
    }
    __syncthreads();
    if (h[0][t])
        atomicAdd(&st->hist[0][t], h[0][t]);
    if (!same && h[1][t])
        atomicAdd(&st->hist[1][t], h[1][t]);
}

__global__ __launch_bounds__(plan::kRadixBins) void k6_select_narrow(SelectState* st, int pass, float* __restrict__ out)
{
    __shared__ uint32_t scan[plan::kRadixBins];
    const int t = threadIdx.x;
    st += blockIdx.x;
    const uint32_t p[2] = {st->prefix[0], st->prefix[1]}, rk[2] = {st->rank[0], st->rank[1]};
    const bool same = p[0] == p[1];
    uint32_t c[2];
    c[0] = st->hist[0][t];
    c[1] = same ? c[0] : st->hist[1][t];
    __syncthreads();   // every thread has read the state before any thread changes it
    st->hist[0][t] = 0;
    st->hist[1][t] = 0;
    for (int r = 0; r < 2; r++) {
        scan[t] = c[r];
        __syncthreads();
        for (int o = 1; o < plan::kRadixBins; o <<= 1) {   // inclusive prefix sums of the counts
            const uint32_t add = t >= o ? scan[t - o] : 0u;
            __syncthreads();
            scan[t] += add;
            __syncthreads();
        }
        const uint32_t before = scan[t] - c[r];
        if (plan::radix_bin_holds(before, c[r], rk[r])) {   // true in exactly one thread
            const uint32_t np = (p[r] << plan::kRadixBits) | (uint32_t)t;
            st->prefix[r] = np;
            st->rank[r] = rk[r] - before;
            if (pass == plan::kRadixPasses - 1)
                out[2 * blockIdx.x + r] = __uint_as_float(plan::radix_key_inverse(np));
        }
        __syncthreads();
    }
}

// ---- levels, table, output --------------------------------------------------------------------------------------------

// copy_and_scale_uchar's (x - a) * b or ImageConverter_uchar::copy_and_scale's x * a + b, then cvRound + saturate_cast<uchar>
__device__ __forceinline__ int level_of(float x, float a, float b, int affine)
{
    const float y = affine ? __fadd_rn(__fmul_rn(x, a), b) : __fmul_rn(__fsub_rn(x, a), b);
    return plan::render_level(rintf(y));
}

// The caller's table [256][3] bytes as one dword per level in LDS (b | g << 8 | r << 16): one LDS read per pixel.
__device__ __forceinline__ void load_table(uint32_t* lut, const uint8_t* __restrict__ lut_bgr)
{
    for (int i = threadIdx.x; i < 256; i += blockDim.x)
        lut[i] = (uint32_t)lut_bgr[3 * i] | ((uint32_t)lut_bgr[3 * i + 1] << 8) | ((uint32_t)lut_bgr[3 * i + 2] << 16);
}

// Four adjacent BGR pixels (e[j]: 24 bits each): twelve bytes as one three-dword store where the address allows.
__device__ __forceinline__ void store_bgr_quad(uint8_t* __restrict__ out, const uint32_t (&e)[4], int cnt, bool vec)
{
    if (vec) {
        struct alignas(4) W3 {
            uint32_t x, y, z;
        } w;
        w.x = e[0] | (e[1] << 24);
        w.y = (e[1] >> 8) | (e[2] << 16);
        w.z = (e[2] >> 16) | (e[3] << 8);
        *reinterpret_cast<W3*>(out) = w;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (j < cnt) {
            out[3 * j] = (uint8_t)(e[j] & 255u);
            out[3 * j + 1] = (uint8_t)((e[j] >> 8) & 255u);
            out[3 * j + 2] = (uint8_t)((e[j] >> 16) & 255u);
        }
}

// ---- plane render ---------------------------------------------------------------------------------------------------------
struct RenderArgs {
    const float* planes;
    const uint8_t* valid;   // nullable, same strides
    const uint8_t* lut_bgr; // device copy of the caller's table
    uint8_t* out;           // [n_planes][rows][cols][3]
    long long plane_stride, row_stride;
    int rows, cols, quads_per_row;
    float a, b;             // plan::render_consts
    const float2* ab;       // nullable: plan::render_consts of every plane, (a, b)[n_planes], in place of a, b
    int affine;             // RSLF_RENDER_AFFINE
    int zero_value;         // RSLF_MASK_ZERO_VALUE (else RSLF_MASK_BLACK)
    VolView vol;            // the shadow cut's volume (C > 0)
    int slice_epi, index;   // RSLF_SLICE_*: plane k is view index + k, or scanline index + k
    float shadow_level;
};

// One lane = four adjacent pixels of one row of plane blockIdx.y.  C = 0: no shadow cut; C = 1 / 3: the volume's channels.
// The slab's rows are [pitch][C] floats with pitch a multiple of 64 beyond U, so the 4 C floats of a lane's shadow test
// are C aligned 16-byte loads in either slice kind, in range also for a row's last, partial quad.
template <int C, bool VEC>
__global__ __launch_bounds__(plan::kRenderBlock) void k6_render_planes(RenderArgs A)
{
    __shared__ uint32_t lut[256];
    load_table(lut, A.lut_bgr);
    __syncthreads();
    const int k = blockIdx.y;
    const long long q = (long long)blockIdx.x * plan::kRenderBlock + threadIdx.x;
    if (q >= (long long)A.rows * A.quads_per_row)
        return;
    const int r = (int)(q / A.quads_per_row), u0 = (int)(q - (long long)r * A.quads_per_row) * 4;
    const int cnt = min(4, A.cols - u0);
    const long long o = (long long)k * A.plane_stride + (long long)r * A.row_stride + u0;
    const float a = A.ab ? A.ab[k].x : A.a, b = A.ab ? A.ab[k].y : A.b;
    float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t m = 0xffffffffu;   // a byte per pixel
    if (VEC) {
        const float4 f = *reinterpret_cast<const float4*>(A.planes + o);
        x[0] = f.x, x[1] = f.y, x[2] = f.z, x[3] = f.w;
        if (A.valid)
            m = *reinterpret_cast<const uint32_t*>(A.valid + o);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (j < cnt) {
                x[j] = A.planes[o + j];
                if (A.valid && !A.valid[o + j])
                    m &= ~(255u << (8 * j));
            }
    }
    uint32_t e[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const bool ok = ((m >> (8 * j)) & 255u) != 0;
        const float xv = (!ok && A.zero_value) ? 0.0f : x[j];   // rslf_fine_to_coarse.hpp:458-459: before the level is taken
        e[j] = lut[level_of(xv, a, b, A.affine)];
        if (!ok && !A.zero_value)                                // :356, :514: black after the look-up
            e[j] = 0;
    }
    if (C > 0) {   // :360-372, :466-481, applied last
        const int s = A.slice_epi ? r : A.index + k, v = A.slice_epi ? A.index + k : r;
        const float4* rad = reinterpret_cast<const float4*>(A.vol.row(v, s) + (long long)u0 * C);
        float f[4 * (C > 0 ? C : 1)];
#pragma unroll
        for (int i = 0; i < C; i++) {
            const float4 g = rad[i];
            f[4 * i] = g.x, f[4 * i + 1] = g.y, f[4 * i + 2] = g.z, f[4 * i + 3] = g.w;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float nrm = C == 1 ? norm1(f[j]) : norm3(f[C * j], f[C * j + (C > 1 ? 1 : 0)], f[C * j + (C > 2 ? 2 : 0)]);
            if (nrm < A.shadow_level)
                e[j] = 0;
        }
    }
    store_bgr_quad(A.out + (((long long)k * A.rows + r) * A.cols + u0) * 3, e, cnt, VEC);
}

// ---- EPI line painter -----------------------------------------------------------------------------------------------------
// get_coloured_epi of the pile and single-EPI classes (rslf_depth_computation.hpp:588-617, :392-413): every masked
// column u of scanline v draws, in view s, the column u + (int)std::round(depth * (float)(s_hat - s)), and a target
// keeps the source with the greatest depth (the occlusion map's strict `<`, so of equal depths the first, i.e. smallest,
// u: the loop's sequential meaning; under OpenMP the reference races).  One workgroup per (s, scanline): the z-buffer is
// an atomicMax in LDS on (orderable depth bits << 32 | ~u), then one pass colours the winners with the SHIFT formula
// over the min and max of ALL of the scanline's depths (:587 scales best_depth_u alone, masked or not).
// Dynamic LDS (plan::epi_lines_lds_bytes): keys [U] | 16 floats of the range reduction | table [256].
__global__ __launch_bounds__(plan::kEpiLinesBlock) void k6_epi_lines(const float* __restrict__ depth_vu, const uint8_t* __restrict__ mask_vu,
                                                                    int U, int s_hat, int v_first, const uint8_t* __restrict__ lut_bgr,
                                                                    uint8_t* __restrict__ out, int vec)
{
    extern __shared__ unsigned long long zbuf[];
    float* red = reinterpret_cast<float*>(zbuf + U);
    uint32_t* lut = reinterpret_cast<uint32_t*>(red + 16);
    const int t = threadIdx.x, s = blockIdx.x, S = gridDim.x;
    const long long line = (long long)(v_first + blockIdx.y) * U;
    const float* depth = depth_vu + line;
    const uint8_t* mask = mask_vu + line;
    load_table(lut, lut_bgr);
    float mn = INFINITY, mx = -INFINITY;
    for (int u = t; u < U; u += plan::kEpiLinesBlock) {
        zbuf[u] = 0ull;
        const float d = depth[u];
        mn = fminf(mn, d);
        mx = fmaxf(mx, d);
    }
    for (int o = kWave / 2; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if ((t & (kWave - 1)) == 0) {
        red[t / kWave] = mn;
        red[4 + t / kWave] = mx;
    }
    __syncthreads();
    mn = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    mx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    const float slope = (float)(s_hat - s);
    for (int u = t; u < U; u += plan::kEpiLinesBlock) {
        if (!mask[u])
            continue;
        const float d = depth[u];
        if (!(d > -INFINITY))   // NaN, or minus infinity, which is never above the occlusion map's start
            continue;
        const float rf = roundf(__fmul_rn(d, slope));   // halves away from zero
        if (!(fabsf(rf) < 1.0e9f))                      // beyond every row (the reference's int conversion is undefined there)
            continue;
        const int target = u + (int)rf;
        if (target < 0 || target >= U)
            continue;
        const float dk = d == 0.0f ? 0.0f : d;          // -0.0f and +0.0f are equal depths
        const unsigned long long key = ((unsigned long long)plan::radix_key(__float_as_uint(dk)) << 32) | (uint32_t)~(uint32_t)u;
        atomicMax(&zbuf[target], key);
    }
    __syncthreads();
    const float a = mn, b = (float)(255.0 / ((double)mx - (double)mn));
    uint8_t* row = out + ((long long)blockIdx.y * S + s) * U * 3;
    for (int q = t; 4 * q < U; q += plan::kEpiLinesBlock) {
        uint32_t e[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int c = 4 * q + j;
            const unsigned long long key = c < U ? zbuf[c] : 0ull;
            e[j] = 0;   // no line reaches the pixel: black
            if (key)
                e[j] = lut[level_of(depth[~(uint32_t)key], a, b, 0)];
        }
        store_bgr_quad(row + 12ll * q, e, min(4, U - 4 * q), vec != 0);
    }
}

}  // namespace rslf
