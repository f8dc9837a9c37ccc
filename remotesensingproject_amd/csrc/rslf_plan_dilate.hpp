// The host-side decisions of the dilation along u (rslf_volume_dilate_u, rslf_planes_undilate_u; rslf_dilate.hip,
// k16_dilate.hpp): which arguments are arguments, the output width, the weight table, the tile of a workgroup and the source
// segment it stages, the capped grid, and the bytes the step moves.  Host-only like rslf_plan.hpp, which it continues; pure
// functions, g++ compiles it alone; tested by tests/cpp/test_plan_dilate.cpp.  The per-sample rule itself is
// k16_dilate_rule.hpp, shared with the kernel.
#pragma once

#include <limits.h>
#include <stddef.h>

#include "k16_dilate_rule.hpp"

namespace rslf {
namespace plan {

constexpr int kDilateBlock = 256;                      // threads of a workgroup
constexpr int kDilateLane = 4;                         // consecutive floats of the flattened output row a lane writes: 16 bytes
constexpr int kDilateTile = kDilateBlock * kDilateLane;   // floats of a tile
// Floats of LDS a workgroup stages the source segment of its tile in.  The segment is widest for f = 1, C = 3, six taps:
// 1023 / f + C + C * T floats of columns (dilate_stage, k16_dilate_rule.hpp) plus up to 3 + 3 for the 16-byte alignment of its two ends.
constexpr int kDilateStage = 1056;
// The grid cap of a memory-bound kernel: 256 CUs x 8 workgroups; the tiles beyond are strided over.
constexpr unsigned kDilateGridCap = 2048;
constexpr unsigned kUndilateRowCap = 65535;            // grid.y of the undilate kernels, the rows beyond strided over

// What rslf_dilated_width and rslf_volume_dilate_u refuse of their numbers, in the order they look.
enum DilateArg { kDilateOk = 0, kDilateBadWidth, kDilateBadFactor, kDilateBadKind, kDilateTooWide };
// U' of (U, f); *U_out is written only for kDilateOk.  kDilateTooWide: U' + 64 does not fit an int.
inline DilateArg dilated_width(int U, int f, int* U_out)
{
    if (U < 1)
        return kDilateBadWidth;
    if (!dilate_factor_ok(f))
        return kDilateBadFactor;
    const long long w = dilate_width(U, f);
    if (w > (long long)INT_MAX - 64)
        return kDilateTooWide;
    if (U_out)
        *U_out = (int)w;
    return kDilateOk;
}
inline DilateArg dilate_args(int U, int f, int kind, int* U_out)
{
    const DilateArg a = dilated_width(U, f, U_out);
    if (a != kDilateOk)
        return a;
    return dilate_kind_ok(kind) ? kDilateOk : kDilateBadKind;
}

// The source width of a dilated one: U with f * (U - 1) + 1 == U_dilated, or 0 when there is none.
inline int undilated_width(int U_dilated, int f)
{
    if (U_dilated < 1 || !dilate_factor_ok(f) || (U_dilated - 1) % f != 0)
        return 0;
    return (U_dilated - 1) / f + 1;
}

// A row is its pitch * C floats, pad included (the kernel writes the pad's zeros): tiles of kDilateTile floats.
inline long long dilate_row_floats(int pitch_out, int C) { return (long long)pitch_out * C; }
inline long long dilate_tiles_per_row(int pitch_out, int C) { return (dilate_row_floats(pitch_out, C) + kDilateTile - 1) / kDilateTile; }
inline long long dilate_tiles(long long rows, int pitch_out, int C) { return rows * dilate_tiles_per_row(pitch_out, C); }
inline unsigned dilate_grid(long long tiles) { return tiles < 1 ? 0u : (tiles < (long long)kDilateGridCap ? (unsigned)tiles : kDilateGridCap); }

// The source segment tile `t` of a row stages (dilate_stage, k16_dilate_rule.hpp: the kernel runs the same function).
inline DilateStage dilate_tile_stage(long long t, int U, int U_out, int C, int f, int taps, int pitch_in)
{
    return dilate_stage((int)(t * kDilateTile), kDilateTile, U, U_out, C, f, taps, pitch_in * C);
}

// The undilate kernels' grid: x over the columns, y over the rows (capped).
inline unsigned undilate_grid_x(int U) { return U < 1 ? 0u : (unsigned)((U + kDilateBlock - 1) / kDilateBlock); }
inline unsigned undilate_grid_y(size_t rows) { return rows < 1 ? 0u : (rows < kUndilateRowCap ? (unsigned)rows : kUndilateRowCap); }

}  // namespace plan
}  // namespace rslf
