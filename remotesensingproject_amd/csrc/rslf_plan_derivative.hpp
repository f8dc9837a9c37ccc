// The pure decisions of the derivative channels (rslf_volume_derivative_channels, rslf_derivative_channels_dense;
// rslf_derivative.hip, k17_derivative.hpp): which weights are weights, how a row splits into peeled ends and 16-byte
// groups, the tile of a workgroup and the row segment it stages, the capped grid, and the bytes the step moves.  No HIP;
// g++ compiles it alone; every function is constexpr, so the kernel runs the same ones; tested by
// tests/cpp/test_plan_derivative.cpp.  The per-pixel rule itself is k17_derivative_rule.hpp.
#pragma once

#include <limits.h>
#include <stddef.h>

#include "k17_derivative_rule.hpp"

namespace rslf {
namespace plan {

constexpr int kDerivBlock = 256;                        // threads of a workgroup
constexpr int kDerivLane = 4;                           // consecutive columns a lane owns: one 16-byte load, three 16-byte stores
constexpr int kDerivTile = kDerivBlock * kDerivLane;    // columns of a tile
constexpr int kDerivStage = kDerivTile + 2 * kDerivLane;   // floats of LDS: the tile's columns from stage[4] on (16-byte slots), a halo column at stage[3] and one after them
constexpr unsigned kDerivGridCap = 2048;                // a memory-bound kernel: 256 CUs x 8 workgroups, the tiles beyond strided over

// A weight of the volume and dense entries: finite and > 0.  (x == x && x - x == 0: finite, without <cmath>'s overloads.)
constexpr bool derivative_finite(float x) { return x == x && x - x == 0.0f; }
constexpr bool derivative_weight_ok(float w) { return derivative_finite(w) && w > 0.0f; }
// The pyramid's option: 0 is off, otherwise a weight.
constexpr bool derivative_option_ok(float w) { return derivative_finite(w) && w >= 0.0f; }
// The cap of the dense entry on float elements: max(m, 0) of some m, so not a NaN and not negative (+inf caps nothing).
constexpr bool derivative_hi_ok(float hi) { return hi == hi && hi >= 0.0f; }

// What the entries refuse of a source's shape, in the order they look.
enum DerivativeArg { kDerivOk = 0, kDerivBadShape, kDerivTooLarge };
// A dense level [V][S][U]: its 3 * V * S * U output floats are indexed by long long, a row's 3 * U by int.
constexpr DerivativeArg derivative_shape(int V, int S, int U)
{
    if (V < 1 || S < 1 || U < 1)
        return kDerivBadShape;
    if ((long long)U > (INT_MAX - 64) / kDerivativeChannels || (long long)V * S > (long long)INT_MAX)
        return kDerivTooLarge;
    return kDerivOk;
}

// How the columns [0, U) of a row split: `head` columns handled one by one, then `body` columns in groups of four whose
// first float is 16-byte aligned in the source and in the result, then `tail` columns one by one.
struct DerivativeRow {
    int head, body, tail;
};
// The volume form: rows start at multiples of 256 bytes and are `pitch` columns long (a multiple of 64), pad included: all body.
constexpr DerivativeRow derivative_row_volume(int pitch) { return DerivativeRow{0, pitch, 0}; }
// The raw form: the row starts `row_first` floats (row * U) after a base; column u of it is 16-byte aligned in the source
// (float row_first + u) and in the result (float 3 * (row_first + u)) exactly when row_first + u is a multiple of 4 and
// both bases are 16-byte aligned.  Bases that are not: the whole row is peeled.
constexpr DerivativeRow derivative_row_raw(long long row_first, int U, bool bases_aligned)
{
    if (!bases_aligned)
        return DerivativeRow{U, 0, 0};
    const int lead = (int)((4 - row_first % 4) % 4);
    const int head = lead < U ? lead : U;
    const int body = (U - head) / kDerivLane * kDerivLane;
    return DerivativeRow{head, body, U - head - body};
}
constexpr int derivative_peeled(const DerivativeRow& r) { return r.head + r.tail; }
// The k-th peeled column of a row, k in [0, head + tail).
constexpr int derivative_peeled_column(const DerivativeRow& r, int k) { return k < r.head ? k : r.body + k; }

// Tiles of a row: its body in runs of kDerivTile columns; a row without a body still has tile 0, which also does the peel.
// A launch gives every row derivative_tiles_per_row(pitch) or, in the raw form, (U) of them -- no row's body is longer -- and
// a tile at or beyond the end of its row's body (other than tile 0) has nothing to do.
constexpr int derivative_tiles_per_row(int body) { return body < 1 ? 1 : (body + kDerivTile - 1) / kDerivTile; }
constexpr bool derivative_tile_works(const DerivativeRow& r, int t) { return t == 0 || t * kDerivTile < r.body; }
constexpr unsigned derivative_grid(long long tiles) { return tiles < 1 ? 0u : (tiles < (long long)kDerivGridCap ? (unsigned)tiles : kDerivGridCap); }

// The first column c0 of tile t and the stage: column c of the row sits at stage[c - c0 + 4].  Lane `tid` fills the slot of
// its own group, columns c0 + 4 tid .. + 3, where the group lies inside the body; one lane fills the halo before them with
// column max(c0 - 1, 0) and one the float after the tile's last group, column derivative_stage_end, clamped to U - 1.  A lane
// then reads two floats of it: the column before its group and the column after.
constexpr int derivative_tile_first(const DerivativeRow& r, int t) { return r.head + t * kDerivTile; }
constexpr int derivative_stage_end(const DerivativeRow& r, int c0)
{
    const int body_end = r.head + r.body;
    return c0 + kDerivTile < body_end ? c0 + kDerivTile : body_end;
}
constexpr int derivative_stage_index(int column, int c0) { return column - c0 + kDerivLane; }

// Bytes the step reads and writes, for a comparison with a copy: the source three times over (the row itself and the rows
// v - 1 and v + 1; the caches serve most of the second and third) is not counted -- once in, three channels out.
constexpr size_t derivative_bytes(size_t floats_in, size_t floats_out) { return (floats_in + floats_out) * sizeof(float); }

}  // namespace plan
}  // namespace rslf
