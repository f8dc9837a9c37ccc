// Host-side planning of the gfx950 EPI depth scan: pure functions, no HIP, no device state.
//
// Everything the library decides on the host before it queues work lives here, so that it can be compiled with g++
// alone and unit-tested under AddressSanitizer / UBSan on a box without a GPU (tests/cpp/test_plan.cpp,
// tests/test_plan_cpu.py): which scanlines a device and a chunk take and with what halo, in which order a sweep
// visits the views, how many hypothesis groups and row blocks a scan launch uses and how many records that costs,
// how the streaming kernel's LDS is shared out, which copies a chunk's upload needs, how the pyramid's levels are
// sized, and in which order the devices of a sharded sweep wait for one another.  The .hip translation units only
// turn these plans into launches and copies.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/rslf_hip.h"   // RSLF_SCAN_*

namespace rslf {

// cv::getStructuringElement result as one bit row per kernel row (k <= 31); the device side is k1_morph_pass
struct MorphElement {
    int k;
    unsigned rows[31];
};

namespace plan {

// ---- constants of the launch shapes -------------------------------------------------------------------------------

constexpr int kScanWavesPerTile = 4;                               // waves of a scan workgroup = hypothesis chunks per tile
constexpr size_t kPartialRecordBytes = 32;                         // sizeof(rslf::Partial), checked in k2_scan.hpp
constexpr size_t kPartialBudget = (size_t)256 << 20;               // bytes of (tile, group, lane) records per grouped scan launch
constexpr size_t kAutoGroupBudget = (size_t)96 << 20;              // ... of which the AUTOMATIC groups of short register launches may take
constexpr int kPackedItemTarget = 2048;                            // packed launches: (tile, group) items the device aims for
constexpr int kSweepGroups = 32;                                   // workgroups sharing a packed tile on a sweep's sparse visits
constexpr int kStreamGroups = 16;                                  // dense launches of the streaming kernel: workgroups per tile
constexpr size_t kStreamSmallEpiBytes = (size_t)2 << 20;           // ... 2 or 3 where a scanline's EPI is at most this (half an XCD's L2)
constexpr size_t kScanOffsetTableBytes = (size_t)48 << 10;        // LDS kernels: the waves' view-offset tables fit this
constexpr int kRowSplitMin = 64;                                   // packed launches of stream-class volumes: rows with at least this many pixels go as row tiles
constexpr int kChipGroups = 8;                                     // ... of the on-chip kernel: half the records, same speed (profiles/r03_k2_variants.md)
constexpr size_t kStreamLdsBytes = (size_t)80 << 10;               // dynamic LDS of one streaming workgroup (two per CU)
constexpr size_t kStagingBudget = (size_t)256 << 20;               // device staging buffer of the chunked host upload
constexpr int kMinSpatialDim = 10;                                 // _MIN_SPATIAL_DIM, rslf_fine_to_coarse.hpp:8

// ---- the on-chip kernel's ladder (k2_chip.hpp) -----------------------------------------------------------------------
// A rung = how many views sit in the AGPR tier (NA) and the LDS tier (NL) behind the 64 of the VGPR tier; three more are
// fetched ahead on every pass.  The tiers fill in that order as the view count grows.  A volume runs on the SMALLEST rung
// that holds all its views, the missing ones padded with samples that contribute nothing (~1 % of a hypothesis each; a
// view beyond a rung, fetched again on every pass, costs 3.5 %) -- so the rungs are 8 views apart.  The top rung is
// BASELINE.json's c5 (201 views), which has its own unpadded instantiation, and one with a ragged tail for 202..220.
// The lists are per translation unit (rslf_chip_a/b/c.hip: each instantiation is ~20 s of hipcc).
constexpr int kChipNV = 64, kChipNAMax = 84, kChipNLMax = 50, kChipAhead = 3;
constexpr int kChipPadMax = 10;                                    // a rung holds at most this many views more than the volume has
constexpr int kChipBestFloats = 4 * 64;                            // a wave's running index and rbar (ChipBest)
constexpr size_t kChipLdsBytes = (size_t)160 << 10;                // one workgroup per CU may take all of it
constexpr int kChipMaxS = 220;                                     // beyond, the per-pass fetches cost more than the streaming kernel's tail
#ifndef RSLF_CHIP_LADDER_A
#define RSLF_CHIP_LADDER_A(X) X(84, 32) X(84, 40) X(84, 50)
#define RSLF_CHIP_LADDER_B(X) X(84, 0) X(84, 8) X(84, 16) X(84, 24)
#define RSLF_CHIP_LADDER_C(X) X(60, 0) X(68, 0) X(76, 0)
#endif
#define RSLF_CHIP_LADDER(X) RSLF_CHIP_LADDER_C(X) RSLF_CHIP_LADDER_B(X) RSLF_CHIP_LADDER_A(X)
#ifndef RSLF_CHIP_FIRST_S
#define RSLF_CHIP_FIRST_S 123   // fewer views: the streaming kernel's two waves per SIMD are faster (profiles/r04_k2_variants.md section 9)
#endif
struct ChipRung {
    int na, nl;
    constexpr int views() const { return kChipNV + na + kChipAhead + nl; }
};
#define RSLF_CHIP_RUNG_(NA, NL) ChipRung{NA, NL},
constexpr ChipRung kChipLadder[] = {RSLF_CHIP_LADDER(RSLF_CHIP_RUNG_)};   // ascending
#undef RSLF_CHIP_RUNG_
constexpr int kChipRungs = (int)(sizeof(kChipLadder) / sizeof(kChipLadder[0]));
constexpr int kChipTopS = kChipLadder[kChipRungs - 1].views();
constexpr int kChipMinS = RSLF_CHIP_FIRST_S > kChipLadder[0].views() - kChipPadMax ? RSLF_CHIP_FIRST_S : kChipLadder[0].views() - kChipPadMax;
constexpr bool chip_ladder_ok()
{
    for (int i = 1; i < kChipRungs; i++)
        if (kChipLadder[i].views() <= kChipLadder[i - 1].views() || kChipLadder[i].views() - kChipLadder[i - 1].views() > kChipPadMax)
            return false;
    return true;
}
static_assert(chip_ladder_ok(), "rungs ascend, and a volume is never padded by more than kChipPadMax views");

// the rung a volume of S views runs on: the smallest that holds them all; beyond the top rung, the top rung (-1: none)
inline int chip_rung_for(int S)
{
    if (S < kChipMinS || S > kChipMaxS)
        return -1;
    for (int i = 0; i < kChipRungs; i++)
        if (kChipLadder[i].views() >= S)
            return i;
    return kChipRungs - 1;
}
// the wave's table of view offsets: one entry per view of the volume or of the rung, whichever is more
constexpr int chip_table_floats(int S, int rung_views) { return ((S > rung_views ? S : rung_views) + 3) & ~3; }
// floats of dynamic LDS per wave: [view offsets][NL samples x 3 channels x 64 lanes][running best, 4 x 64] -- and no less
// than the epilogue's block, which reuses the region's head
constexpr int chip_wave_floats(int S, const ChipRung& r)
{
    return chip_table_floats(S, r.views()) + r.nl * 3 * 64 + kChipBestFloats < 2 * (64 + 6 * 32)
               ? 2 * (64 + 6 * 32)
               : chip_table_floats(S, r.views()) + r.nl * 3 * 64 + kChipBestFloats;
}
// the kernel takes RGB volumes that have a rung and whose per-wave LDS share fits
inline bool chip_takes(int S, int C)
{
    if (C != 3)
        return false;
    const int r = chip_rung_for(S);
    return r >= 0 && (size_t)chip_wave_floats(S, kChipLadder[r]) * 4 * kScanWavesPerTile <= kChipLdsBytes;
}

// Register-variant slot counts compiled into the library (multiples of 8), per channel count: those that run at two or
// more waves per SIMD.  Beyond them the streaming / on-chip kernels take over (k2_scan.hpp).
#ifndef RSLF_SPAD_LIST_1CH
#define RSLF_SPAD_LIST_1CH(X) X(8) X(16) X(24) X(32) X(40) X(48) X(56) X(64) X(72) X(80) X(88) X(96) X(104) X(112) X(120) X(128) \
    X(144) X(160) X(176) X(192)
#endif
#ifndef RSLF_SPAD_LIST_3CH
#define RSLF_SPAD_LIST_3CH(X) X(8) X(16) X(24) X(32) X(40) X(48)
#endif

// Smallest compiled slot count >= S (0 = none: another kernel runs).
inline int pick_spad(int S, int C)
{
    int best = 0;
#define RSLF_PICK(N) \
    if (N >= S && best == 0) best = N;
    if (C == 1) {
        RSLF_SPAD_LIST_1CH(RSLF_PICK)
    } else if (C == 3) {
        RSLF_SPAD_LIST_3CH(RSLF_PICK)
    }
#undef RSLF_PICK
    return best;
}

// ---- small reference rules ----------------------------------------------------------------------------------------

// dc.hpp:490-494 (pile) / :303-311 (single EPI): an s_hat outside the views means the middle one
inline int resolve_s_hat(int s_hat, int S)
{
    if (s_hat < 0 || s_hat > S - 1)
        return (int)std::floor((0.0 + S) / 2);
    return s_hat;
}

// core.hpp:584: `for (int i = 0; i < par_mean_shift_max_iter; i++)` with a FLOAT bound
inline int mean_shift_passes(float max_iter)
{
    int n = 0;
    while ((float)n < max_iter && n < (1 << 20))
        n++;
    return n;
}

// core.hpp:981-990: the centre view, then outwards, alternating (an even view count never reaches view 0)
inline std::vector<int> sweep_order(int S)
{
    std::vector<int> order;
    if (S < 1)
        return order;
    const int s_mid = (int)std::floor(S / 2.0);
    order.push_back(s_mid);
    for (int off = 1; off < S - s_mid; off++) {
        order.push_back(s_mid + off);
        if (s_mid - off > -1)
            order.push_back(s_mid - off);
    }
    return order;
}

inline int sweep_view_after(int S, int s_hat)
{
    const std::vector<int> order = sweep_order(S);
    for (size_t i = 0; i + 1 < order.size(); i++)
        if (order[i] == s_hat)
            return order[i + 1];
    return -1;
}

// ---- the line confidence of a sweep (k7_line_conf.hpp; core.hpp:1032-1081 under _USE_LINE_CONFIDENCE_SCORE) ----------
// 0: not computed (the default build); 1: computed and carried, the gate stays the edge mask (what the macro compiles
// to: the gating branches sit behind an `#elseif` typo, core.hpp:1099); 2: computed, carried and gating (what those
// branches say).
constexpr int kLineConfOff = 0, kLineConfAsBuilt = 1, kLineConfGate = 2;

inline bool line_conf_mode_ok(int mode) { return mode >= kLineConfOff && mode <= kLineConfGate; }

// Which plane gates the propagation of a visit (core.hpp:1097-1103): the #ifdef chain gives C_d the gate whenever
// use_disp_confidence_score is set; C_l has it in mode 2 alone; else the edge mask.
enum SweepGate { kGateEdgeMask = 0, kGateDispConf = 1, kGateLineConf = 2 };
inline SweepGate sweep_gate(bool use_disp_confidence_score, int line_mode)
{
    if (use_disp_confidence_score)
        return kGateDispConf;
    return line_mode == kLineConfGate ? kGateLineConf : kGateEdgeMask;
}

// Which plane a level of the pyramid reads its validity from (get_valid_depths_mask_s_v_u, dc.hpp:893-915, asked for by the
// next level's bounds, f2c.hpp:185-186, and by the fusion, :312): everything (C_e > -1) with accept_all; C_l > the line
// threshold where the line confidence gates (mode 2, and C_d does not come first in the #ifdef chain); else C_e > the edge
// threshold.  This is the table of the entries that take no validity rule (RSLF_F2C_VALID_COMPAT): under
// use_disp_confidence_score it reads C_e, never C_d (:902) -- f2c_validity_by_rule below has that branch.
enum F2cValidity { kValidAll = 0, kValidLineConf = 1, kValidEdgeConf = 2, kValidDispConf = 3 };
inline F2cValidity f2c_validity(bool accept_all, bool use_disp_confidence_score, int line_mode)
{
    if (accept_all)
        return kValidAll;
    return sweep_gate(use_disp_confidence_score, line_mode) == kGateLineConf ? kValidLineConf : kValidEdgeConf;
}

// The validity of a kept run (rslf_f2c_run_host) under its rule.  Compat: f2c_validity, row for row.  Reference: the whole
// #ifdef chain of dc.hpp:893-915 -- accept_all, else C_d > the disparity threshold under use_disp_confidence_score (:902),
// else C_l > the line threshold in the gating mode (:904), else C_e > the edge threshold (:906).
constexpr int kF2cValidCompat = 0, kF2cValidReference = 1;
inline bool f2c_validity_rule_ok(int rule) { return rule == kF2cValidCompat || rule == kF2cValidReference; }
inline F2cValidity f2c_validity_by_rule(bool accept_all, bool use_disp_confidence_score, int line_mode, int rule)
{
    if (rule != kF2cValidReference)
        return f2c_validity(accept_all, use_disp_confidence_score, line_mode);
    if (accept_all)
        return kValidAll;
    if (use_disp_confidence_score)
        return kValidDispConf;
    return line_mode == kLineConfGate ? kValidLineConf : kValidEdgeConf;
}

// K7 runs before the claims only where the claims gate on its plane; it then needs the filtered plane first, from a median
// pass of its own.  Where C_d or the edge mask gates, K7 follows median + claims (which leaves the filtered plane).
inline bool line_conf_before_claims(bool use_disp_confidence_score, int mode)
{
    return sweep_gate(use_disp_confidence_score, mode) == kGateLineConf;
}

// Launches rslf_sweep_visit_finish queues.  Off: median + claims, apply.  K7 after the claims: one more.  K7 before them: the
// median alone, K7, median + claims, apply.
inline int line_conf_finish_launches(bool use_disp_confidence_score, int mode)
{
    if (mode == kLineConfOff)
        return 2;
    return line_conf_before_claims(use_disp_confidence_score, mode) ? 4 : 3;
}

// Bytes of the sweep-long K(r - rbar) columns [V][S][U] (core.hpp:975-979) and of a visit's arg-max plane [V][U]; 0 when off
// or when a dimension is not positive.
inline size_t line_conf_columns_bytes(int mode, int V, int S, int U)
{
    if (mode == kLineConfOff || V < 1 || S < 1 || U < 1)
        return 0;
    return (size_t)V * (size_t)S * (size_t)U * sizeof(float);
}

inline size_t line_conf_argmax_bytes(int mode, int V, int U)
{
    if (mode == kLineConfOff || V < 1 || U < 1)
        return 0;
    return (size_t)V * (size_t)U * sizeof(int32_t);
}

// cv::getStructuringElement(shape, Size(k, k)) with the default anchor, as OpenCV 3.x builds it (imgproc/src/morph.cpp):
// RECT every column; CROSS the anchor row entirely, elsewhere the anchor column; ELLIPSE the columns
// [c - dx, c + dx + 1), dx = cvRound(c * sqrt((r*r - dy*dy) / (r*r))), r = c = k/2, dy = i - r.
inline MorphElement structuring_element(int shape, int k)
{
    MorphElement el;
    el.k = k;
    const int r = k / 2, c = k / 2;
    const double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
    for (int i = 0; i < 31; i++)
        el.rows[i] = 0;
    for (int i = 0; i < k && i < 31; i++) {
        int j1 = 0, j2 = 0;
        if (shape == 0 || (shape == 1 && i == k / 2)) {
            j2 = k;
        } else if (shape == 1) {
            j1 = k / 2;
            j2 = j1 + 1;
        } else {
            const int dy = i - r;
            if (std::abs(dy) <= r) {
                const int dx = (int)std::lrint(c * std::sqrt((r * r - dy * dy) * inv_r2));
                j1 = std::max(c - dx, 0);
                j2 = std::min(c + dx + 1, k);
            }
        }
        for (int j = j1; j < j2 && j < 31; j++)
            el.rows[i] |= 1u << j;
    }
    return el;
}

// cvRound(x * 0.5): ties to even (fine_to_coarse_core.cpp:47-48)
inline void f2c_level_dims(int V, int U, int* V2, int* U2)
{
    *V2 = (int)std::lrint(V * 0.5);
    *U2 = (int)std::lrint(U * 0.5);
}

struct LevelDims {
    int V, U;
};

// The pyramid of FineToCoarse's constructor (rslf_fine_to_coarse.hpp:130-154): levels while both sides exceed
// _MIN_SPATIAL_DIM and the depth limit allows (max_depth < 1: no limit).
inline std::vector<LevelDims> f2c_pyramid(int V, int U, int max_depth)
{
    std::vector<LevelDims> levels;
    if (max_depth < 1)
        max_depth = 1 << 30;
    int dim_v = V, dim_u = U, counter = 0;
    while (dim_v > kMinSpatialDim && dim_u > kMinSpatialDim && counter < max_depth) {
        counter++;
        levels.push_back(LevelDims{dim_v, dim_u});
        int v2, u2;
        f2c_level_dims(dim_v, dim_u, &v2, &u2);
        if (v2 < 1 || u2 < 1)
            break;
        dim_v = v2;
        dim_u = u2;
    }
    return levels;
}

// Pixels per row of a volume's slab: > U (the second lerp tap of u = U - 1 lands on zeros), a multiple of 64.
inline int volume_pitch(int U) { return ((U + 1 + 63) / 64) * 64; }
inline size_t volume_bytes(int V, int S, int U, int C)
{
    if (V < 1 || S < 1 || U < 1 || C < 1)
        return 0;
    return (size_t)V * (size_t)S * (size_t)C * (size_t)volume_pitch(U) * sizeof(float);
}

// Device bytes a kept fine-to-coarse run (rslf_f2c_run) holds for one level: disparities, C_e and C_d (float), validity
// (a byte), C_l with a line mode, and the level's volume where volumes are kept ...
inline size_t f2c_kept_level_bytes(int S, int C, LevelDims d, int line_mode, bool keep_volumes)
{
    if (S < 1 || d.V < 1 || d.U < 1)
        return 0;
    const size_t n = (size_t)S * (size_t)d.V * (size_t)d.U;
    const size_t float_planes = line_mode == kLineConfOff ? 3 : 4;
    return n * (float_planes * sizeof(float) + 1) + (keep_volumes ? volume_bytes(d.V, S, d.U, C) : 0);
}
// ... and for the whole pyramid, with the fused map (float) and the fused validity (a byte) at the finest size.
inline size_t f2c_kept_bytes(int S, int C, const std::vector<LevelDims>& dims, int line_mode, bool keep_volumes)
{
    if (dims.empty() || S < 1)
        return 0;
    size_t total = (size_t)S * (size_t)dims[0].V * (size_t)dims[0].U * (sizeof(float) + 1);
    for (const LevelDims& d : dims)
        total += f2c_kept_level_bytes(S, C, d, line_mode, keep_volumes);
    return total;
}

// ---- the selective median (core.hpp:663-718; k3_median.hpp) -------------------------------------------------------

constexpr int kMedianBlock = 256;          // pixels of one scanline per workgroup
constexpr int kMedianNetMaxSide = 11;      // window sides up to this sort their slots in registers
constexpr int kMedianTileMaxSide = 31;     // ... up to this keep the window tile in LDS (one predicate word per window row)
constexpr int kMedianMaxSize = 1 << 30;    // sizes past this are refused as invalid (v + width must stay an int)

// core.hpp:686: `int width = (a_size-1)/2;` -- C++ division truncates, so size 0 is the 1 x 1 window too
inline int median_width(int size) { return (size - 1) / 2; }

// floats of dynamic LDS a median workgroup needs for window half-width w: depths + C radiance planes of the tile
inline size_t median_lds_bytes(int w, int C)
{
    return (size_t)(1 + C) * (size_t)(2 * w + 1) * (size_t)(kMedianBlock + 2 * w) * sizeof(float);
}

struct MedianPlan {
    int w;             // window half-width
    int mode;          // > 0: window side of the register network; 0: LDS tile + radix select; < 0: global radix select
    size_t lds_bytes;
};

inline MedianPlan median_plan(int size, int C)
{
    MedianPlan m;
    m.w = std::max(0, median_width(size));
    const int side = 2 * m.w + 1;
    m.mode = side <= kMedianNetMaxSide ? side : side <= kMedianTileMaxSide ? 0 : -1;
    m.lds_bytes = m.mode >= 0 ? median_lds_bytes(m.w, C) : 0;
    return m;
}

// norm<T>(x) < eps (src/rslf_types.cpp:80-91; core.hpp:703-706, :1116) as ONE compare, exactly.
//   1 channel:  float(double(|x|) * 1.73205080757) < eps   -- non-decreasing in |x|  <=>  |x| < a1
//   3 channels: float(sqrt(s)) < eps, s = the double sum of squares  -- non-decreasing in s  <=>  s < s3
// a1 / s3 = the smallest non-negative float / double for which the test FAILS, found by bisection over bit patterns
// (ordered like the values).  eps <= 0 or NaN: nothing passes (a1 = s3 = 0).  The kernels then need no double multiply
// (1 channel) and no double square root (3 channels) per window pixel.
struct NormThreshold {
    float a1;
    double s3;
};

inline bool norm1_below(float ax, float eps) { return (float)((double)ax * 1.73205080757) < eps; }
inline bool norm3_below(double s, float eps) { return (float)std::sqrt(s) < eps; }

inline NormThreshold norm_threshold(float eps)
{
    NormThreshold t;
    t.a1 = 0.0f;
    t.s3 = 0.0;
    if (norm1_below(0.0f, eps)) {
        uint32_t lo = 0u, hi = 0x7F800000u;   // test(lo) true; test(+inf) false: float(inf) < eps never holds
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            float x;
            memcpy(&x, &mid, sizeof x);
            if (norm1_below(x, eps))
                lo = mid;
            else
                hi = mid;
        }
        memcpy(&t.a1, &hi, sizeof hi);
    }
    if (norm3_below(0.0, eps)) {
        uint64_t lo = 0u, hi = 0x7FF0000000000000ull;
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            double x;
            memcpy(&x, &mid, sizeof x);
            if (norm3_below(x, eps))
                lo = mid;
            else
                hi = mid;
        }
        memcpy(&t.s3, &hi, sizeof hi);
    }
    return t;
}

// ---- scanline partitions ------------------------------------------------------------------------------------------

// rows either side of a block that must be recomputed (pile path) or exchanged (sweep) for the block's own rows to come
// out exact: the median reads +-(size-1)/2 rows (core.hpp:686), and through the optional opening +-2*(k/2) rows more
// (core.hpp:759-768)
inline int median_halo(int median_filter_size) { return std::max(0, median_width(median_filter_size)); }
inline int halo_rows(int median_filter_size, int opening_size)
{
    return median_halo(median_filter_size) + (opening_size > 1 ? 2 * (opening_size / 2) : 0);
}

struct RowBlock {
    int a, b;     // owned rows [a, b) of the whole field
    int lo, hi;   // held / computed rows: owned + halo, clipped to the field
};

// block i of n over V scanlines: contiguous, sizes differ by at most one, together they cover [0, V) exactly
inline RowBlock row_block(int V, int i, int n, int halo)
{
    RowBlock r;
    r.a = (int)((long long)V * i / n);
    r.b = (int)((long long)V * (i + 1) / n);
    r.lo = std::max(0, r.a - halo);
    r.hi = std::min(V, r.b + halo);
    return r;
}

// A sharded sweep's blocks must be able to fill their neighbours' halo rows from rows they own: fewer devices otherwise.
inline int sweep_devices_for(int V, int n_devices, int halo)
{
    int nd = std::max(1, n_devices);
    while (nd > 1 && V / nd < std::max(1, halo))
        nd--;
    return nd;
}

// Chunks of one device's rows [r0, r1) on the pipelined host path.  A given size: uniform.  Automatic (chunk_rows <= 0):
// a short first chunk so that the kernels start early (its upload is the one copy nothing hides), then two large ones
// (stacked input; scattered input, which is gathered into pinned memory first, takes a middling second chunk and pieces
// of about rows/3.5) -- a chunk's scan is a grid of its own, and a grid of 5.4 rounds of workgroups pays for 6.
inline std::vector<RowBlock> chunk_plan(int r0, int r1, int V, int halo, int chunk_rows, bool scattered)
{
    std::vector<RowBlock> chunks;
    const int rows = r1 - r0;
    if (rows <= 0)
        return chunks;
    std::vector<int> sizes;
    if (chunk_rows > 0) {
        for (int a = 0; a < rows; a += chunk_rows)
            sizes.push_back(std::min(chunk_rows, rows - a));
    } else {
        int left = rows;
        const int first = std::min(left, std::max(32, (rows + 15) / 16));
        sizes.push_back(first);
        left -= first;
        if (left > 0 && scattered) {   // gathered through pinned memory first: smaller steps keep the kernels fed
            const int second = std::min(left, std::max(32, (rows + 7) / 8));
            sizes.push_back(second);
            left -= second;
        }
        if (left > 0) {
            // the chunk before has to cover the next one's upload with its scan
            const int n = scattered ? std::max(1, (int)std::lround(left / (rows / 3.5))) : (left > 2 * first ? 2 : 1);
            for (int i = 0; i < n; i++) {
                const int sz = (left + (n - i) - 1) / (n - i);
                sizes.push_back(sz);
                left -= sz;
            }
        }
    }
    int a = r0;
    for (int sz : sizes) {
        if (sz <= 0)
            continue;
        RowBlock c;
        c.a = a;
        c.b = a + sz;
        c.lo = std::max(0, c.a - halo);
        c.hi = std::min(V, c.b + halo);
        chunks.push_back(c);
        a += sz;
    }
    return chunks;
}

inline int max_held_rows(const std::vector<RowBlock>& chunks)
{
    int m = 0;
    for (const RowBlock& c : chunks)
        m = std::max(m, c.hi - c.lo);
    return m;
}

// worker t of nt over `rows` items: [first, last)
inline void split_range(int rows, int t, int nt, int* first, int* last)
{
    *first = (int)((long long)rows * t / nt);
    *last = (int)((long long)rows * (t + 1) / nt);
}

// ---- host copies --------------------------------------------------------------------------------------------------

// Number of maximal runs of EPIs that follow one another in host memory among ptrs[0..rows): each run is one 1-D copy.
// Rows with a stride (row_stride != row_bytes) are a run each.
inline int count_runs(const void* const* ptrs, int rows, size_t row_stride_bytes, size_t row_bytes, size_t epi_bytes)
{
    if (rows <= 0)
        return 0;
    int runs = 1;
    for (int i = 1; i < rows; i++)
        if (row_stride_bytes != row_bytes || (const char*)ptrs[i] != (const char*)ptrs[i - 1] + epi_bytes)
            runs++;
    return runs;
}

// Are the EPIs [r0, r1) scattered over the heap (a Vec<Mat>) rather than stacked in one array?
inline bool epis_scattered(const void* const* ptrs, int r0, int r1, size_t row_stride_bytes, size_t row_bytes, size_t epi_bytes)
{
    if (row_stride_bytes != row_bytes)
        return true;
    for (int i = r0 + 1; i < r1; i++)
        if (ptrs[i] && ptrs[i - 1] && (const char*)ptrs[i] != (const char*)ptrs[i - 1] + epi_bytes)
            return true;
    return false;
}

// A chunk goes through the pinned staging buffer when it is broken into more than 8 runs AND the buffer holds it
// (the buffer is sized from the scattered-ness of the device's own rows; a chunk's halo rows can add breaks of their
// own, so the capacity is checked per chunk -- ADVICE r2).
inline bool use_pinned_gather(int runs, int rows, size_t epi_bytes, size_t pin_cap)
{
    return runs > 8 && pin_cap > 0 && (size_t)rows * epi_bytes <= pin_cap;
}

// The gather itself: EPIs [i0, i1) of `epis` (S rows of row_bytes, `stride` bytes apart) as dense rows at
// dst + i * S * row_bytes -- one copy per EPI where the rows are dense already, else one per row (a pad is never read).
inline void gather_epis(char* dst, const void* const* epis, int i0, int i1, int S, size_t row_bytes, size_t stride)
{
    const size_t epi_bytes = (size_t)S * row_bytes;
    for (int i = i0; i < i1; i++) {
        const char* e = (const char*)epis[i];
        char* o = dst + (size_t)i * epi_bytes;
        if (stride == row_bytes)
            memcpy(o, e, epi_bytes);
        else
            for (int r = 0; r < S; r++)
                memcpy(o + (size_t)r * row_bytes, e + (size_t)r * stride, row_bytes);
    }
}

// rows per pass of the chunked host upload through the bounded device staging buffer
inline int staging_chunk_rows(size_t epi_bytes, int V, size_t budget = kStagingBudget)
{
    const size_t c = std::max<size_t>(1, budget / std::max<size_t>(1, epi_bytes));
    return (int)std::min<size_t>(c, (size_t)std::max(1, V));
}

// ---- result planes of one chunk, carved from one block ------------------------------------------------------------

struct PlaneLayout {   // byte offsets into the block, for n pixels and C channels
    size_t Ce, Cd, depth, raw, score, rbar, idx, mask, counts, bytes;
};

inline PlaneLayout plane_layout(size_t n, int C, int count_rows)
{
    PlaneLayout q;
    q.Ce = 0;
    q.Cd = q.Ce + n * 4;
    q.depth = q.Cd + n * 4;
    q.raw = q.depth + n * 4;
    q.score = q.raw + n * 4;
    q.rbar = q.score + n * 4;
    q.idx = q.rbar + n * 4 * (size_t)C;
    q.mask = q.idx + n * 4;
    q.counts = (q.mask + n + 15) & ~(size_t)15;
    q.bytes = q.counts + (size_t)count_rows * sizeof(int);
    return q;
}

// The eight [V][U] result planes of a pile step as pointers: a carved block on the device, or the caller's planes.
struct PilePlanes {
    float *Ce, *Cd, *depth, *raw, *score, *rbar;
    int32_t* idx;
    uint8_t* mask;
};

inline PilePlanes carve(char* base, size_t n, int C)
{
    const PlaneLayout o = plane_layout(n, C, 0);
    PilePlanes q;
    q.Ce = (float*)(base + o.Ce);
    q.Cd = (float*)(base + o.Cd);
    q.depth = (float*)(base + o.depth);
    q.raw = (float*)(base + o.raw);
    q.score = (float*)(base + o.score);
    q.rbar = (float*)(base + o.rbar);
    q.idx = (int32_t*)(base + o.idx);
    q.mask = (uint8_t*)(base + o.mask);
    return q;
}

// The one enumeration of the planes, in the order the C-ABI lists them: f(host plane, device plane, bytes per pixel) for
// every plane the caller wants (a NULL host plane is skipped).  f returns 0 to go on; anything else ends the enumeration
// and is returned.
template <typename F>
inline int for_each_plane(const PilePlanes& host, const PilePlanes& dev, int C, F f)
{
    const struct {
        void* host;
        const void* dev;
        size_t bytes_per_pixel;
    } planes[8] = {{host.Ce, dev.Ce, 4},     {host.mask, dev.mask, 1},   {host.Cd, dev.Cd, 4},   {host.depth, dev.depth, 4}, {host.rbar, dev.rbar, 4 * (size_t)C},
                   {host.idx, dev.idx, 4},   {host.score, dev.score, 4}, {host.raw, dev.raw, 4}};
    for (const auto& q : planes)
        if (q.host)
            if (int rc = f(q.host, q.dev, q.bytes_per_pixel))
                return rc;
    return 0;
}

// ---- scan launches ------------------------------------------------------------------------------------------------

// largest fraction below 1 that cannot round a position up to the next integer: 1 - ulp(largest position the scan forms)
inline float stream_frac_max(int U)
{
    int e = 0;
    (void)std::frexp((float)U + 2.0f, &e);   // U + 2 < 2^e
    return 1.0f - std::ldexp(1.0f, std::max(e - 24, -24));
}

// The pixel-per-wave kernel of sparse launches (k2_reg.hpp, k2_scan_reg_px): a pixel's hypotheses sit in the LANES of 1, 2
// or 4 waves (lane slot + k * 64 * waves), so what matters is how many lanes a pixel keeps busy.  Returns the number of
// waves per pixel with the best lane use (the larger on ties: finer items), or 0 when no choice reaches 60 %.
inline int px_waves(int dim_d)
{
    int best = 0;
    double best_use = 0.0;
    for (int w = 1; w <= kScanWavesPerTile; w *= 2) {
        const int lanes = 64 * w, iters = (dim_d + lanes - 1) / lanes;
        const double use = (double)dim_d / ((double)iters * lanes);
        if (use >= best_use - 1e-12) {
            best_use = use;
            best = w;
        }
    }
    return best_use >= 0.6 ? best : 0;
}

struct ScanRequest {
    int V, U, S, C, dim_d;
    // the kernel (choose_scan_kernel)
    int spad;              // register kernel's slot count, 0 = none
    bool use_stream;       // streaming kernel
    bool use_chip;         // on-chip kernel (k2_chip.hpp): one workgroup per CU, row tiles as the streaming kernel's, never packed
    int chip_wave_floats;  // its dynamic LDS per wave, in floats
    int reg_waves;         // waves per SIMD of the register kernel (scan_reg_waves), 0 if unknown
    int num_cus;           // compute units of the device, 0 if unknown
    int ctx_groups;        // groups the caller asked for (the sweep's sparse visits), >= 1
    bool ctx_packed;       // the caller asked for one packed pixel list
    int precompacted;      // 0: the scan compacts; 1: row lists are in place (K1); 2: the packed list is (sweep)
    int force_groups;      // debug hooks: 0 / -1 = automatic
    int force_packed;
    int px_mode;           // pixel-per-wave kernel for packed launches of a register kernel: -1 automatic, 0 never, 1 whenever it can run
    int stream_groups;     // 0 = kStreamGroups
    int stream_share;      // 63-pixel row tiles (shared taps): 0 never, 1 where the re-gathered tail is long enough to pay for them, 2 always
    size_t stream_lds_bytes;
    int tap_table, scalar_taps;   // register row kernels that have them: lane-invariant lerp taps from the per-hypothesis table / row-exact hypotheses' taps as scalars from the per-launch table (0: off; A/B and tests)
};

struct ScanPlan {
    int kind;              // RSLF_SCAN_*: the kernel that runs
    int spad;              // ... the register kernel's slot count, 0 = another kernel
    int groups;            // workgroups sharing one tile's hypotheses
    bool packed;           // one packed list over all scanlines
    bool packed_adapt;     // the device settles the group count from the list length
    int px_waves;          // > 0: the pixel-per-wave kernel takes the packed list, this many waves per pixel (no groups, no records)
    int tap_table, scalar_taps;   // the register row kernel may take its taps from the table / the launch gets a row-exact table (the request's hooks, both on for the second; row tiles only)
    int tile_w;            // 63 or 64 entries per row tile
    int tiles_per_row;
    int rows_per_launch;   // grouped row-tile launches go by blocks of scanlines
    size_t records;        // 32-byte records the launches need (0 when groups == 1)
    size_t tickets;        // one int per tile of a launch
    // streaming kernel
    int stream_nres;       // resident prefix of the instantiation that runs (k2_stream.hpp)
    int stream_park;       // samples per lane parked in LDS
    int stream_wave_floats;
    size_t lds_bytes;
};

inline int stream_resident_hi(int C, int nres_1ch, int nres_rgb) { return C == 1 ? nres_1ch : nres_rgb; }

// What the device headers fix for a volume of S views x C channels, passed in so that this header stays host-only
struct ScanKernelFacts {
    int reg_waves;   // scan_reg_waves(pick_spad(S, C), C) (k2_reg.hpp), 0 where no register kernel has the slots
    int nres;        // stream_resident_for(S, C) (k2_stream.hpp): the streaming kernel's resident prefix
    int nres_px;     // stream_px_resident_for(S, C): ... of its pixel-per-wave form
};

// LDS kernels take radiances in [0, 1e6]: max(R, 0) == R, and the 1e30 sentinel dwarfs them
inline bool scan_range_ok(float min_value, float max_value) { return min_value >= 0.0f && max_value <= 1.0e6f; }

// Which kernel scans r's volume (S views x C channels): fills r's kernel fields.  The register kernel where S is within its
// compiled slot counts; the streaming kernel for any S whose offset table fits the LDS; both need radiances in range and
// linear interpolation.  Instead of the streaming kernel, the on-chip one for the RGB view counts it has a rung for
// (chip_takes: more views than two waves per SIMD hold on chip), on a row-tile launch with one hypothesis grid for all
// pixels (`dense_uniform`, what it is written for).  Otherwise the generic kernel.  `force_scan` (debug hook, the parity
// tests exercise every variant on small cases): 1 the generic kernel, 2 the streaming kernel wherever it can run.
inline void choose_scan_kernel(ScanRequest* r, bool in_range, bool linear, int force_scan, bool dense_uniform, const ScanKernelFacts& f)
{
    const bool lds_ok = in_range && linear && force_scan != 1 && (size_t)kScanWavesPerTile * r->S * sizeof(float) <= kScanOffsetTableBytes;
    r->spad = lds_ok && force_scan == 0 ? pick_spad(r->S, r->C) : 0;
    r->use_chip = lds_ok && r->spad == 0 && dense_uniform && force_scan != 2 && chip_takes(r->S, r->C);
    r->use_stream = lds_ok && r->spad == 0 && !r->use_chip;
    r->chip_wave_floats = r->use_chip ? chip_wave_floats(r->S, kChipLadder[chip_rung_for(r->S)]) : 0;
    r->reg_waves = r->spad ? f.reg_waves : 0;
}

// The streaming kernel's LDS per wave: the S view offsets (rounded up to 4) and as many batches of parked samples as the
// workgroup's share leaves room for (never past the end of the views).  Returns the parked samples per lane.
inline int stream_park_for(int S, int C, int nres, size_t stream_lds_bytes)
{
    if (nres <= 0)
        return 0;
    const int batch = C == 1 ? 8 : 4;
    const size_t s4 = ((size_t)S + 3) & ~(size_t)3;
    size_t room = stream_lds_bytes / kScanWavesPerTile / sizeof(float);   // floats per wave
    room -= std::min(room, s4);
    int park = (int)(room / ((size_t)C * 64));
    park = std::min(park, S - nres);
    park = std::max(park, 0);
    return park - park % batch;
}

// Shared taps (63-pixel row tiles, one texel load per sample, the right tap from lane + 1) halve the loads of the samples
// that are gathered again on EVERY pass -- and cost a lane per tile.  They pay where that tail is long: 109 of 201 views at
// c5 (+9 %); at 100 views RGB the tail is 8 samples and plain 64-pixel tiles are 6 % faster (47.5 vs 44.7 ms,
// profiles/r04_k2_variants.md).  Rule: the tail is at least a quarter of the views.
inline bool stream_shares_taps(int S, int nres, int park) { return 4 * (S - nres - park) >= S; }

// `nres` = the streaming kernel's resident prefix for this volume (stream_resident_for), needed only with use_stream;
// `nres_px` = the prefix of its pixel-per-wave form (stream_px_resident_for; -1: the same).
inline ScanPlan plan_scan(const ScanRequest& r, int nres, int nres_px = -1)
{
    ScanPlan p;
    const size_t n = (size_t)r.V * r.U;
    int groups = std::max(1, r.ctx_groups);
    bool packed = r.ctx_packed;
    // the streaming kernel's dense launches share tiles so that what an XCD's workgroups gather from fits its L2
    if ((r.use_stream || r.use_chip) && groups == 1 && !packed) {
        groups = r.stream_groups > 0 ? r.stream_groups : kStreamGroups;
        // the on-chip kernel reads a tile's samples once per workgroup whatever their number; fewer workgroups per tile leave
        // fewer records -- unless the launch is then only a few rounds of workgroups
        const long long tiles = (long long)r.V * ((r.U + 62) / 63);
        if (r.use_chip && r.stream_groups <= 0 && (r.num_cus <= 0 || tiles * kChipGroups >= 8LL * r.num_cus))
            groups = kChipGroups;
        // The streaming kernel's groups are there for the XCD's L2.  Where one scanline's EPI (all its views) is a small part
        // of it and the launch has workgroups to spare, two or three groups are enough and every group fewer is a record
        // not written and merged: 100 views RGB x 1146 px (1.4 MB), 120 hypotheses, dense: 8 groups 44.9 ms, 4 43.4, 3 41.0,
        // 2 41.6, 1 43.3 (profiles/r04_k2_variants.md section 12).  Three where the hypotheses divide evenly over its 12 waves.
        if (r.use_stream && r.stream_groups <= 0 && (size_t)r.S * r.U * r.C * sizeof(float) <= kStreamSmallEpiBytes) {
            const int few = r.dim_d % (3 * kScanWavesPerTile) == 0 ? 3 : 2;
            if (r.num_cus <= 0 || tiles * few >= 16LL * r.num_cus)
                groups = few;
        }
    }
    // A dense launch of a register kernel whose grid is only a few rounds of workgroups pays for its last, partly empty
    // round: sharing each tile's hypotheses among 2-8 workgroups makes the rounds shorter and more numerous -- as long
    // as a wave keeps at least eight hypotheses and ~256 (hypothesis, view) pairs.
    if (r.spad && groups == 1 && !packed && r.num_cus > 0 && r.reg_waves > 0) {
        const long long tiles = (long long)r.V * ((r.U + 63) / 64);
        const long long resident = (long long)r.num_cus * r.reg_waves;
        // (and the records stay a modest scratch: the groups are a convenience here, not the kernel's locality)
        while (groups < 8 && tiles * groups < 40 * resident && r.dim_d >= 8 * kScanWavesPerTile * 2 * groups &&
               (long long)(r.dim_d / (kScanWavesPerTile * 2 * groups)) * r.S >= 256 &&
               (size_t)tiles * (size_t)(groups * 2) * 64 * kPartialRecordBytes <= kAutoGroupBudget)
            groups *= 2;
    }
    if (r.force_groups > 0)
        groups = std::min(64, r.force_groups);
    if (r.force_packed >= 0)
        packed = r.force_packed != 0;
    if (n > (size_t)INT32_MAX || r.precompacted == 1)
        packed = false;   // entry counts are ints; precompacted: the row lists are what K1 wrote
    if (r.precompacted == 2)
        packed = true;    // the previous visit's apply pass left the packed list and its length
    // enough hypotheses to share out?
    while (groups > 1 && r.dim_d < 2 * kScanWavesPerTile * groups)
        groups /= 2;

    // Packed launches of a register or streaming kernel: lanes own hypotheses, a wave owns a pixel (the gather of a sparse
    // list is then 64 neighbouring taps of one scanline instead of 64 scanlines) -- no hypothesis groups, no records
    int px_w = 0;
    if (packed && (r.spad || r.use_stream) && !r.use_chip && r.px_mode != 0) {
        px_w = px_waves(r.dim_d);
        if (px_w == 0 && r.px_mode == 1)
            px_w = 1;
    }
    if (px_w && r.use_stream && nres_px >= 0)
        nres = nres_px;
    p.stream_nres = r.use_stream ? nres : 0;
    const int park_early = r.use_stream ? stream_park_for(r.S, r.C, nres, r.stream_lds_bytes) : 0;
    const bool share = r.use_chip ? r.stream_share != 0
                                  : r.use_stream && (r.stream_share == 2 || (r.stream_share == 1 && stream_shares_taps(r.S, nres, park_early)));
    p.tile_w = (share && !packed) ? 63 : 64;
    // 63-entry tiles: a row's last tile takes up to 64 entries (scan_tile)
    p.tiles_per_row = p.tile_w == 63 ? std::max(1, (r.U + 61) / 63) : (r.U + p.tile_w - 1) / p.tile_w;
    p.packed_adapt = packed && !r.use_stream && !r.use_chip;
    p.rows_per_launch = r.V;
    if (groups > 1 && !packed) {
        const size_t per_row = (size_t)p.tiles_per_row * groups * 64 * kPartialRecordBytes;
        p.rows_per_launch = (int)std::min<size_t>((size_t)r.V, std::max<size_t>(1, kPartialBudget / per_row));
    }
    if (packed && (r.use_stream || r.use_chip))
        while (groups > 1 && ((n + 63) / 64) * groups * 64 * kPartialRecordBytes > kPartialBudget)
            groups /= 2;
    p.px_waves = px_w;
    p.tap_table = (r.spad && !packed && r.tap_table) ? 1 : 0, p.scalar_taps = (p.tap_table && r.scalar_taps) ? 1 : 0;
    p.spad = r.spad;
    p.kind = r.spad ? (px_w ? RSLF_SCAN_REG_PX : RSLF_SCAN_REG)
             : r.use_chip ? RSLF_SCAN_CHIP
             : r.use_stream ? (px_w ? RSLF_SCAN_STREAM_PX : RSLF_SCAN_STREAM) : RSLF_SCAN_GENERIC;
    if (px_w) {
        groups = 1;
        p.packed_adapt = false;
    }
    p.groups = groups;
    p.packed = packed;
    p.records = 0;
    p.tickets = 0;
    if (groups > 1) {
        const size_t tiles_all = (n + 63) / 64;
        const size_t tiles_max = !packed ? (size_t)p.rows_per_launch * p.tiles_per_row
                                         : p.packed_adapt ? std::min<size_t>(tiles_all, kPackedItemTarget / 2) : tiles_all;
        p.records = (packed && p.packed_adapt) ? std::min<size_t>(tiles_all * groups, kPackedItemTarget) * 64 : tiles_max * groups * 64;
        p.tickets = tiles_max;
    }
    p.stream_park = 0;
    p.stream_wave_floats = 0;
    p.lds_bytes = 0;
    if (r.use_stream) {
        // LDS per wave: the S view offsets (rounded up to 4) and as many batches of parked samples as the workgroup's
        // share leaves room for (never past the end of the views)
        const size_t s4 = ((size_t)r.S + 3) & ~(size_t)3;
        const int park = park_early;
        p.stream_park = park;
        p.stream_wave_floats = (int)(s4 + (size_t)park * r.C * 64);
        p.stream_wave_floats = std::max(p.stream_wave_floats, 2 * (64 + (3 + r.C) * 32));   // room for the wave's EpilogueBlock
        p.lds_bytes = (size_t)kScanWavesPerTile * p.stream_wave_floats * sizeof(float);
    }
    if (r.use_chip) {
        p.stream_wave_floats = r.chip_wave_floats;
        p.lds_bytes = (size_t)kScanWavesPerTile * r.chip_wave_floats * sizeof(float);
    }
    return p;
}

// Row split (sparse visits of stream-class volumes): the rows of the packed list that hold at least this many pixels go as
// ROW tiles -- the streaming kernel's dense form, reading its tiles straight from the packed list -- and the pixel-per-wave
// launch takes the rest; which rows each scans is settled on the device, from the rows' counts.  `hook` = the row_split
// debug key: 0 off, 1 the default threshold, larger = that many pixels.  0: the launch is not split.
inline int row_split_min(const ScanRequest& r, const ScanPlan& p, int hook)
{
    return r.use_stream && p.px_waves > 0 && hook != 0 ? (hook > 1 ? hook : kRowSplitMin) : 0;
}

// ... the request of its row-tile launches: the lists are in place, and the groups are the launch's parallelism (sparse
// rows), not the dense rule's few
inline ScanRequest row_split_request(ScanRequest r)
{
    r.ctx_packed = false;
    r.ctx_groups = 1;
    r.precompacted = 1;
    r.force_packed = 0;
    if (r.stream_groups <= 0)
        r.stream_groups = kStreamGroups;
    return r;
}

struct ScanLaunch {
    int v0;               // first scanline of the launch's row tiles (0 for a packed list)
    int logical_blocks;   // (tile, group) items: `groups` workgroups per tile, their waves split the hypotheses
    int per_xcd;          // ... dealt to each XCD
    unsigned grid;        // workgroups launched
};

// The launches of a scan of V x U pixels, in order.  Row tiles: one launch per block of rows_per_launch scanlines, the
// scanlines dealt to the XCDs in turn, every XCD ceil(rows / 8) of them (xcd_logical_block_rows).  A packed list: one launch
// of at most ceil(V*U/64) tiles -- the device knows how many -- whose fixed grid strides over the items (k2_scan.hpp): ~4
// workgroups per CU cover any occupancy (the pixel-per-wave kernel's items are 4 / px_waves pixels each).  False when a
// launch would have more than 2^30 items; *bad_tiles is then its tile count.
inline bool scan_launches(int V, int U, const ScanPlan& p, std::vector<ScanLaunch>* out, long long* bad_tiles)
{
    out->clear();
    const size_t n = (size_t)V * U;
    for (int v0 = 0; v0 < V; v0 += p.rows_per_launch) {
        const int rows = std::min(p.rows_per_launch, V - v0);
        const long long tiles = p.packed ? (long long)((n + 63) / 64) : (long long)rows * p.tiles_per_row;
        if (tiles * p.groups > (long long)1 << 30) {
            *bad_tiles = tiles;
            return false;
        }
        ScanLaunch l;
        l.v0 = v0;
        l.logical_blocks = (int)(tiles * p.groups);
        l.per_xcd = p.packed ? (l.logical_blocks + 7) / 8 : ((rows + 7) / 8) * p.tiles_per_row * p.groups;
        const long long px_items = ((long long)n * p.px_waves + kScanWavesPerTile - 1) / kScanWavesPerTile;
        l.grid = p.px_waves ? (unsigned)std::min<long long>(px_items, 2048)
                 : p.packed ? (unsigned)std::min<long long>(tiles * p.groups, 1024)
                            : (unsigned)(l.per_xcd * 8);
        out->push_back(l);
        if (p.packed)
            break;
    }
    return true;
}

// rslf_depth1d_pile_run computes edge confidence and compacts the mask into row lists in ONE launch when nothing sits
// between them: no opening of the mask (core.hpp:759-768), row tiles, entry counts that fit an int
inline bool fuse_k1_compaction(int opening_size, int force_packed, size_t n_pixels)
{
    return opening_size <= 1 && force_packed != 1 && n_pixels <= (size_t)INT32_MAX;
}

// The records and tickets a sweep reserves before its first visit, so that none allocates in the middle of the sequence:
// what its sparse visits ask for (`sparse`: their request) and the row tiles of their row split
inline void sweep_reserve(const ScanRequest& sparse, const ScanKernelFacts& f, int row_split_hook, size_t* records, size_t* tickets)
{
    const ScanPlan p = plan_scan(sparse, f.nres, f.nres_px);
    *records = p.records;
    *tickets = p.tickets;
    if (row_split_min(sparse, p, row_split_hook)) {
        const ScanPlan q = plan_scan(row_split_request(sparse), f.nres);
        *records = std::max(*records, q.records);
        *tickets = std::max(*tickets, q.tickets);
    }
}

// ---- score rows (k2_scores.hpp, rslf_scores.hip): the scan's score matrix [row of the window][U][dim_d] as an output -----
// A wave parks kScoreRun consecutive hypotheses of its 64 pixels in LDS ([pixel][run + 1], an odd pitch: no bank conflicts
// either way) and writes them out 64 B per pixel and store instruction.  16: 17 KiB of parking + 1 KiB of pixel numbers, which
// with the offset tables stays inside a workgroup's LDS share at every occupancy the register kernels run at (8 per CU: 20 KiB).
constexpr int kScoreRun = 16;
constexpr size_t kScoreLdsLimit = (size_t)64 << 10;   // static LDS of one workgroup
inline int score_run_length(int /*spad*/, int /*C*/) { return kScoreRun; }
// (`table_floats`: floats per slot of the wave's offset table -- 4 with the tap table, else 1; spad == 0: the generic form)
constexpr size_t score_lds_bytes(int spad, int table_floats)
{
    return (size_t)kScanWavesPerTile * (64 * ((size_t)(kScoreRun + 1) * sizeof(float) + sizeof(int)) + (size_t)spad * table_floats * sizeof(float));
}
// The form that serves a request: the register one exactly where choose_scan_kernel gives a slot count (radiances in range,
// linear interpolation, no "force_scan"), else the generic one.  Streaming and on-chip forms are not built.
inline int choose_score_kernel(int S, int C, bool in_range, bool linear, int force_scan, int* spad)
{
    ScanRequest r = {};
    r.S = S, r.C = C;
    choose_scan_kernel(&r, in_range, linear, force_scan, false, ScanKernelFacts{0, 0, 0});
    *spad = r.spad;
    return r.spad ? RSLF_SCAN_REG : RSLF_SCAN_GENERIC;
}
// Row tiles of 64 entries; nothing is merged, so hypothesis groups are free: doubled while the window's tiles are fewer than
// eight rounds of resident workgroups and every wave keeps two hypotheses.  The launches are scan_launches' over the window.
inline ScanPlan score_plan(int kind, int spad, int n_rows, int U, int dim_d, int num_cus, int reg_waves, int force_groups)
{
    ScanPlan p = {};
    p.kind = kind, p.spad = spad, p.tile_w = 64, p.tiles_per_row = (U + 63) / 64;
    const long long tiles = (long long)std::max(1, n_rows) * p.tiles_per_row;
    int groups = 1;
    while (groups < 64 && tiles * groups < 8LL * std::max(1, num_cus) * std::max(1, reg_waves) && dim_d >= 4 * kScanWavesPerTile * groups)
        groups *= 2;
    groups = force_groups > 0 ? std::min(64, force_groups) : groups;
    while (groups > 1 && dim_d < 2 * kScanWavesPerTile * groups) groups /= 2;
    p.groups = groups;
    p.rows_per_launch = (int)std::max<long long>(1, std::min<long long>(std::max(1, n_rows), ((long long)1 << 30) / ((long long)p.tiles_per_row * groups)));
    return p;
}
inline bool score_launches(int v_first, int n_rows, int U, const ScanPlan& p, std::vector<ScanLaunch>* out, long long* bad_tiles)
{
    const bool ok = scan_launches(n_rows, U, p, out, bad_tiles);
    for (ScanLaunch& l : *out) l.v0 += v_first;
    return ok;
}
inline size_t score_offset(int row, int u, int d, int U, int dim_d) { return ((size_t)row * (size_t)U + (size_t)u) * (size_t)dim_d + (size_t)d; }
// scanlines per pass of the host form through a staging buffer of budget_bytes: at least one
inline int score_window_rows(int U, int dim_d, size_t budget_bytes)
{
    const size_t row = std::max<size_t>(1, (size_t)U * (size_t)dim_d * sizeof(float));
    return (int)std::min<size_t>(std::max<size_t>(1, budget_bytes / row), (size_t)INT32_MAX);
}

// ---- one visit of a sweep sharded over several devices of one process ---------------------------------------------
//
// scan on every device; every device fetches its neighbours' boundary rows (needs the neighbour's scan); every device
// finishes (median + propagation) once BOTH neighbours have fetched its rows, because its apply pass rewrites them
// (core.hpp:1119-1121).  One host thread queues the ops in this order; `waits` are the cross-device event waits an op's
// stream makes before it runs (same-device order is the stream's own).
struct VisitOp {
    enum Kind { SCAN, FETCH, FINISH } kind;
    int dev;
    int neighbour;                    // FETCH: the device whose rows are read, else -1
    std::vector<int> wait_scan_of;    // devices whose SCAN event this op waits for
    std::vector<int> wait_fetch_of;   // devices whose (last) FETCH event this op waits for
};

inline std::vector<VisitOp> sweep_visit_schedule(int nd, int h_med)
{
    std::vector<VisitOp> ops;
    for (int i = 0; i < nd; i++)
        ops.push_back(VisitOp{VisitOp::SCAN, i, -1, {}, {}});
    for (int i = 0; i < nd; i++)
        for (int side = 0; side < 2 && h_med > 0; side++) {
            const int k = side == 0 ? i - 1 : i + 1;
            if (k < 0 || k >= nd)
                continue;
            ops.push_back(VisitOp{VisitOp::FETCH, i, k, {k}, {}});
        }
    for (int i = 0; i < nd; i++) {
        VisitOp f{VisitOp::FINISH, i, -1, {}, {}};
        if (i > 0)
            f.wait_fetch_of.push_back(i - 1);
        if (i + 1 < nd)
            f.wait_fetch_of.push_back(i + 1);
        ops.push_back(f);
    }
    return ops;
}

// Local row numbers of a boundary-row fetch: device `d` (block bd) reads h rows owned by its neighbour (block bo).
// side 0: the h rows above d's block = the last h own rows of the block before; side 1: the first h own rows of the next.
inline void fetch_rows(const RowBlock& bd, const RowBlock& bo, int side, int h, int* dst_row, int* src_row)
{
    *dst_row = side == 0 ? (bd.a - bd.lo) - h : (bd.b - bd.lo);
    *src_row = side == 0 ? (bo.b - bo.lo) - h : (bo.a - bo.lo);
}

// ---- K6, the renderers (k6_render.hpp, rslf_render.hip) -----------------------------------------------------------
// The reference's getters (get_coloured_epi, get_disparity_map, get_coloured_depth_maps, ..._pyr) and the converter
// they share (rslf_plot.cpp:41-110).  The functions a kernel calls as well are constexpr: hipcc compiles those for
// both sides, so the kernel and the CPU tests run one definition.

constexpr int kRadixBits = 8;                       // one digit of the radix select
constexpr int kRadixBins = 1 << kRadixBits;
constexpr int kRadixPasses = 32 / kRadixBits;       // histogram passes over the plane, most significant digit first
constexpr int kFitBlock = 256;                      // threads of a fit workgroup, four adjacent pixels per thread and step
constexpr int kFitMaxBlocks = 1024;                 // the fit kernels stride over the plane with at most this many workgroups
constexpr int kRenderBlock = 256;                   // threads of a plane-render workgroup, four adjacent pixels each
constexpr int kEpiLinesBlock = 256;                 // threads of the EPI line painter's workgroup (one (v, s) row)
constexpr int kEpiLinesMaxU = 8000;                 // its z-buffer, one 64-bit key per column, stays below 64 KiB of LDS

// A float's bits as a key whose UNSIGNED order is the float order (negative: all bits flipped; else the sign bit set).
// -0.0f lands directly below +0.0f; NaNs land beyond the infinities on the side of their sign.
constexpr uint32_t radix_key(uint32_t float_bits)
{
    return (float_bits & 0x80000000u) ? ~float_bits : (float_bits | 0x80000000u);
}
constexpr uint32_t radix_key_inverse(uint32_t key)
{
    return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
}
// The digit of `key` that pass `pass` (0 = most significant) counts, and the digits above it.
constexpr uint32_t radix_digit(uint32_t key, int pass)
{
    return (key >> (32 - kRadixBits * (pass + 1))) & (uint32_t)(kRadixBins - 1);
}
constexpr uint32_t radix_prefix(uint32_t key, int pass)
{
    return pass == 0 ? 0u : key >> (32 - kRadixBits * pass);
}
// How a rank narrows to a bin: the keys that share the prefix found so far were counted per digit; `before` of them lie
// in lower bins.  The bin with `count` keys holds the key of rank `rank` (0-based among the counted keys) iff this is
// true, and the rank among that bin's keys is then rank - before.  Exactly one bin holds a rank below the total.
constexpr bool radix_bin_holds(uint32_t before, uint32_t count, uint32_t rank)
{
    return rank >= before && rank - before < count;
}
// The same over a whole histogram (what the narrowing kernel's 256 threads do together): the bin, and the rank within it.
inline int radix_narrow(const uint32_t* hist, uint32_t rank, uint32_t* rank_within)
{
    uint32_t before = 0;
    for (int b = 0; b < kRadixBins; b++) {
        if (radix_bin_holds(before, hist[b], rank)) {
            *rank_within = rank - before;
            return b;
        }
        before += hist[b];
    }
    return -1;   // rank >= number of keys counted
}
// ImageConverter_uchar::fit(img, true), rslf_plot.cpp:75-79: (int)std::floor(q * N), the product in double
inline int quantile_index(double q, int n)
{
    return (int)std::floor(q * n);
}
// ... fit(img, false), :85-95: max = min(mean + 12 * std, true_max) with cv::meanStdDev's mean = sum * (1 / N) and
// std = sqrt(max(sumsq * (1 / N) - mean * mean, 0)), all in double
inline double meanstd_max(double sum, double sumsq, int n, double true_max)
{
    const double scale = 1.0 / n;
    const double mean = sum * scale;
    const double sd = std::sqrt(std::max(sumsq * scale - mean * mean, 0.0));
    return std::min(mean + 12 * sd, true_max);
}
inline int fit_blocks(long long n)   // workgroups of a fit launch over n pixels
{
    const long long quads = (n + 3) / 4;
    return (int)std::max<long long>(1, std::min<long long>((quads + kFitBlock - 1) / kFitBlock, kFitMaxBlocks));
}

// The two float constants a render formula applies per pixel (include/rslf_hip.h: RSLF_RENDER_*): level from
// (x - a) * b for SHIFT (copy_and_scale_uchar, rslf_plot.cpp:52-56: `res -= min` subtracts (float)min, convertTo scales by
// (float)(255.0 / (max - min))), from x * a + b for AFFINE (ImageConverter_uchar::copy_and_scale, :106-107:
// float alpha = 255.0 / (max - min); convertTo(..., alpha, -alpha * min) with the product in double).
struct RenderConsts {
    float a, b;
};
inline RenderConsts render_consts(int affine, double min, double max)
{
    const float alpha = (float)(255.0 / (max - min));
    if (!affine)
        return RenderConsts{(float)min, alpha};
    return RenderConsts{alpha, (float)(-(double)alpha * min)};
}
// cvRound + saturate_cast<uchar> of a level: nearest even, clamped to [0, 255]; a NaN, an infinity or anything beyond
// the int range converts to INT_MIN (cvtss2si) and so saturates to 0.  `rounded` is rintf(y).
constexpr int render_level(float rounded)
{
    return !(rounded > -2147483648.0f && rounded < 2147483648.0f) ? 0 : rounded <= 0.0f ? 0 : rounded >= 255.0f ? 255 : (int)rounded;
}
// Four adjacent pixels per lane as 16-byte loads and three output dwords: every row start must keep the alignment.
inline bool render_vec4_ok(int cols, long long row_stride, long long plane_stride, const void* planes, const void* valid, const void* out)
{
    return cols % 4 == 0 && row_stride % 4 == 0 && plane_stride % 4 == 0 && (uintptr_t)planes % 16 == 0 && (uintptr_t)valid % 4 == 0 &&
           (uintptr_t)out % 4 == 0;
}
inline long long render_quads(int rows, int cols)   // lanes of one plane: four adjacent pixels of a row each
{
    return (long long)rows * ((cols + 3) / 4);
}
inline size_t epi_lines_lds_bytes(int U)   // the z-buffer, 16 floats for the scanline's range, the table as 256 dwords
{
    return (size_t)U * 8 + 16 * 4 + 256 * 4;
}
// Index rules of the getters.  Both run off the end in the reference (which then reads out of bounds); here the
// caller gets -1 and refuses.  std::round: halves away from zero.
// FineToCoarse::get_coloured_depth_maps / _pyr, rslf_fine_to_coarse.hpp:344, :497: (int)std::round(dim_s / 2.0)
inline int centre_plane_index(int n)
{
    const int i = (int)std::round(n / 2.0);
    return (n < 1 || i >= n) ? -1 : i;   // n == 1: round(0.5) == 1 == n
}
// get_coloured_epi_pyr, :451: (int)std::round(1.0 * v * dim_v / m_dim_v_orig_)
inline int scaled_row_index(int v, int dim_v, int dim_v_orig)
{
    if (v < 0 || dim_v < 1 || dim_v_orig < 1 || v >= dim_v_orig)
        return -1;
    const int i = (int)std::round(1.0 * v * dim_v / dim_v_orig);
    return i >= dim_v ? -1 : i;
}

}  // namespace plan
}  // namespace rslf
