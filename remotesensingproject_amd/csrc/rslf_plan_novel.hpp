// The host-side decisions of the novel view (rslf_novel_view; rslf_novel.hip, k15_novel_view.hpp): which arguments are
// arguments, the LDS of a row, the columns a thread owns in the fill scan, the bytes the step has to move -- and novel_row, the
// whole rule for one row by plain loops, the counterpart of consistency_pixel: what the kernel computes in chunks, scans and
// batches, and what the host tests compare it with.  Host-only, pure functions, g++ compiles it alone; tested by
// tests/cpp/test_plan_novel.cpp.  The width cap, the grid and the launches are the warp's (rslf_plan_warp.hpp).
#pragma once

#include <vector>

#include "k15_novel_rule.hpp"
#include "rslf_plan_warp.hpp"

namespace rslf {
namespace plan {

// What rslf_novel_view refuses beyond the warp's own list (warp_args, warp_target_arg, warp_limits), in the order it looks.
enum NovelArg { kNovelOk = 0, kNovelNoParams, kNovelBadSources, kNovelBadTol };
inline NovelArg novel_args(bool have_params, int sources, float tol)
{
    if (!have_params)
        return kNovelNoParams;
    if (sources < 1)
        return kNovelBadSources;
    if (!novel_tol_ok(tol))
        return kNovelBadTol;
    return kNovelOk;
}

// Dynamic LDS of a workgroup: one 64-bit key per column, decoded in place to an entry: no second array.
inline size_t novel_lds_bytes(int U) { return (size_t)U * 8; }

// The fill scan: thread i of the kWarpBlock owns the columns [i * chunk, min(U, (i + 1) * chunk)); 32 at the cap.
inline int novel_chunk(int U) { return (U + kWarpBlock - 1) / kWarpBlock; }

// Stage B of a row as the device does it, thread by thread: partials, the scan over the threads, the second pass.  e: [U]
// entries of codes 0 / 1.
inline void novel_fill_chunked(unsigned long long* e, int U, int max_gap, int nearer)
{
    const int chunk = novel_chunk(U);
    int last[kWarpBlock], first[kWarpBlock];
    for (int i = 0; i < kWarpBlock; i++) {
        const int x0 = i * chunk < U ? i * chunk : U, x1 = x0 + chunk < U ? x0 + chunk : U;
        novel_chunk_partials(e, x0, x1, U, &last[i], &first[i]);
    }
    int before[kWarpBlock], after[kWarpBlock];
    for (int i = 0, m = -1; i < kWarpBlock; i++) {
        before[i] = m;
        m = last[i] > m ? last[i] : m;
    }
    for (int i = kWarpBlock - 1, m = U; i >= 0; i--) {
        after[i] = m;
        m = first[i] < m ? first[i] : m;
    }
    for (int i = 0; i < kWarpBlock; i++) {
        const int x0 = i * chunk < U ? i * chunk : U, x1 = x0 + chunk < U ? x0 + chunk : U;
        novel_chunk_fill(e, x0, x1, U, before[i], after[i], max_gap, nearer);
    }
}

// ... and by the rule's own words: run by run along the row.
inline void novel_fill_runs(unsigned long long* e, int U, int max_gap, int nearer)
{
    novel_chunk_fill(e, 0, U, U, -1, U, max_gap, nearer);
}

// The volume as novel_row reads it: [V][S][pitch][C] floats (the slab's layout); base NULL: none.
struct NovelVolume {
    const float* base;
    long long stride_v, stride_s;
    int C;
    const float* row(int v, int s) const { return base + (long long)v * stride_v + (long long)s * stride_s; }
};

// One pixel of stage C: d its disparity.  colour [C] (NULL with no volume); *taken: a colour was taken from a view.
inline int novel_pixel(const float* depth, const uint8_t* valid, int S, int V, int U, int v, int x, float d, float t, int exclude, int radius,
                       int sources, float tol, float slope, const NovelVolume& vol, float* colour, bool* taken)
{
    const long long plane = (long long)V * U, row = (long long)v * U;
    const int C = vol.base ? vol.C : 0;
    std::vector<float> acc((size_t)C, 0.0f), first((size_t)C, 0.0f);
    float wsum = 0.0f;
    int n_src = 0;
    bool have_first = false;
    WarpWalk walk = warp_walk_start(t, S);
    int s = 0;
    while (n_src < sources && warp_walk_next(&walk, t, S, &s)) {
        if (!warp_in_window(s, t, radius))
            break;
        if (s == exclude)
            continue;
        const NovelTap k = novel_tap(d, s, x, U, t, slope);
        if (!k.in_field)
            continue;
        const long long q = (long long)s * plane + row + k.ur;
        const bool agrees = novel_agrees(depth[q], valid ? valid[q] : (uint8_t)255, d, tol);
        if (!agrees && have_first)
            continue;
        const float g = novel_weight(s, t);
        for (int c = 0; c < C; c++) {
            const float* const E = vol.row(v, s);
            const float sample = novel_lerp(k.w, E[(long long)k.i0 * C + c], E[(long long)k.i1 * C + c]);
            if (!have_first)
                first[(size_t)c] = sample;
            if (agrees) {
                const float gs = g * sample;
                acc[(size_t)c] = acc[(size_t)c] + gs;
            }
        }
        have_first = true;
        if (agrees) {
            wsum = wsum + g;
            n_src++;
        }
    }
    for (int c = 0; c < C; c++)
        colour[c] = n_src > 0 ? acc[(size_t)c] / wsum : first[(size_t)c];
    *taken = n_src > 0 || have_first;
    return n_src;
}

// One row (t, v) by plain loops.  fill / depth_out / n_src: [U]; colour [U][C], err [U] (read only with a volume; err also
// needs t a view); *row_err, *row_cov.  Every output is required here (the entries' planes are each nullable).
inline void novel_row(const float* depth, const uint8_t* valid, int S, int V, int U, int v, float t, int exclude, int radius, int nearer,
                      int max_gap, int sources, float tol, float slope, const NovelVolume& vol, bool want_err, uint8_t* fill, float* depth_out,
                      int32_t* n_src, float* colour, float* err, double* row_err, int32_t* row_cov)
{
    const long long plane = (long long)V * U, row = (long long)v * U;
    // A: the best candidate of every column, by the rule's own order
    std::vector<unsigned long long> e((size_t)U, 0ull);
    std::vector<float> bz((size_t)U, 0.0f), bdist((size_t)U, 0.0f);
    std::vector<int> bs((size_t)U, -1);
    for (int s = 0; s < S; s++)
        for (int u = 0; u < U; u++) {
            const long long q = (long long)s * plane + row + u;
            int x = 0;
            if (!warp_candidate(depth[q], valid ? valid[q] : (uint8_t)255, s, u, U, t, exclude, radius, slope, &x))
                continue;
            const float z = warp_z(depth[q], nearer), dist = warp_distance(s, t);
            if (bs[(size_t)x] < 0 || warp_ahead(z, dist, s, bz[(size_t)x], bdist[(size_t)x], bs[(size_t)x])) {
                bz[(size_t)x] = z, bdist[(size_t)x] = dist, bs[(size_t)x] = s;
                e[(size_t)x] = novel_entry(kNovelHit, warp_float_bits(depth[q]));
            }
        }
    // B
    novel_fill_runs(e.data(), U, max_gap, nearer);
    // C
    const int C = vol.base ? vol.C : 0;
    int tv = (int)t;
    tv = tv < 0 ? 0 : tv >= S ? S - 1 : tv;
    *row_err = 0.0, *row_cov = 0;
    for (int x = 0; x < U; x++) {
        const int code = novel_entry_code(e[(size_t)x]);
        fill[x] = (uint8_t)code;
        depth_out[x] = code == kNovelHole ? 0.0f : novel_entry_depth(e[(size_t)x]);
        n_src[x] = 0;
        for (int c = 0; c < C; c++)
            colour[(long long)x * C + c] = 0.0f;
        if (vol.base && want_err)
            err[x] = 0.0f;
        if (code == kNovelHole)
            continue;
        bool taken = false;
        n_src[x] = novel_pixel(depth, valid, S, V, U, v, x, depth_out[x], t, exclude, radius, sources, tol, slope, vol,
                               vol.base ? colour + (long long)x * C : nullptr, &taken);
        if (vol.base && want_err && taken) {
            err[x] = warp_residual(colour + (long long)x * C, vol.row(v, tv) + (long long)x * C, C);
            if (n_src[x] > 0)
                *row_err += (double)err[x];
        }
        *row_cov += n_src[x] > 0 ? 1 : 0;
    }
}

// The algorithmic bytes: per scanline the window's source rows -- disparity and validity byte -- read once for stage A and
// served from L2 for the gathers of all targets; per target pixel and blended view 2 * C taps, one slab row for err, every
// plane asked for written once.  `views` is the mean number of views a pixel's walk samples (at most `sources`, or the window
// where nobody agrees): the caller measures it (n_src) or bounds it.
struct NovelPlanes {
    bool colour, depth, fill, n_src, err, rows;
};
inline size_t novel_out_bytes_per_cell(const NovelPlanes& p, int C)
{
    return (p.fill ? 1 : 0) + (size_t)4 * ((p.depth ? 1 : 0) + (p.n_src ? 1 : 0) + (p.err ? 1 : 0)) + (p.colour ? (size_t)4 * C : 0);
}
inline size_t novel_bytes(int S_window, int V, int U, int T, int C, bool have_valid, double views, const NovelPlanes& p)
{
    const size_t row = (size_t)V * (size_t)U;
    const size_t in = (size_t)S_window * row * (4 + (have_valid ? 1 : 0));
    const bool vol = p.colour || p.err || p.rows;
    const size_t taps = vol ? (size_t)((double)T * (double)row * views * (double)(8 * C + 4 + (have_valid ? 1 : 0))) : 0;
    const size_t own = p.err || p.rows ? (size_t)T * row * 4 * C : 0;
    return in + taps + own + (size_t)T * row * novel_out_bytes_per_cell(p, C) + (p.rows ? (size_t)T * V * 12 : 0);
}

}  // namespace plan
}  // namespace rslf
