// The pure decisions of the derivative channels (csrc/rslf_plan_derivative.hpp) under -fsanitize=address,undefined: the walk
// k17_derivative_channels makes over a field -- rows, tiles, lanes, the stage, the peeled row ends -- re-enacted on the
// host with the plan's own functions, for every U in 1..300 and a few wide rows, V in 1..3, both forms, aligned and
// unaligned bases: every output float is written exactly once, every load stays inside its row, every stage index lies
// inside the stage and holds the column the rule asks for.  Also the weights, the cap and the shapes the entries refuse.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "rslf_plan_derivative.hpp"

using namespace rslf;
using namespace rslf::plan;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

// One launch over a field of `rows` rows.  pitch > 0: the volume form.  Returns the lanes that wrote a group.
static long long walk(int rows, int U, int pitch, bool bases_aligned)
{
    const int row_in = pitch ? pitch : U;
    const int row_out = row_in * kDerivativeChannels;
    const int tiles_per_row = derivative_tiles_per_row(pitch ? pitch : U);
    const long long tiles = (long long)rows * tiles_per_row;
    CHECK(derivative_grid(tiles) >= 1 && derivative_grid(tiles) <= kDerivGridCap && (long long)derivative_grid(tiles) <= tiles);
    std::vector<int> written((size_t)rows * row_out, 0);
    long long groups = 0;
    for (long long tile = 0; tile < tiles; tile++) {
        const long long row = tile / tiles_per_row;
        const int t = (int)(tile - row * tiles_per_row);
        const DerivativeRow r = pitch ? derivative_row_volume(pitch) : derivative_row_raw(row * U, U, bases_aligned);
        CHECK(r.head >= 0 && r.body >= 0 && r.tail >= 0 && r.body % kDerivLane == 0 && r.head + r.body + r.tail == row_in);
        if (!pitch && bases_aligned) {   // the body's first column is 16-byte aligned, and no more than three columns are peeled at an end
            CHECK(r.head <= 3 && r.tail <= 3);
            CHECK(r.body == 0 || (row * U + r.head) % 4 == 0);
        }
        CHECK(derivative_tiles_per_row(r.body) <= tiles_per_row);
        if (!derivative_tile_works(r, t))
            continue;
        int* out = &written[(size_t)row * row_out];
        const int c0 = derivative_tile_first(r, t);
        const int end = derivative_stage_end(r, c0);
        CHECK(end >= c0 && end <= c0 + kDerivTile && end <= r.head + r.body);
        std::vector<int> stage(kDerivStage, -1);   // the column a slot holds
        const auto put = [&](int index, int column) {
            CHECK(index >= 0 && index < kDerivStage);
            CHECK(column >= 0 && column < row_in);   // the load stays inside the row
            CHECK(stage[(size_t)index] == -1);        // no two lanes fill one slot
            stage[(size_t)index] = column;
        };
        for (int tid = 0; tid < kDerivBlock; tid++) {
            const int u0 = c0 + kDerivLane * tid;
            if (u0 < end) {
                CHECK(u0 + kDerivLane <= r.head + r.body);
                CHECK(derivative_stage_index(u0, c0) % kDerivLane == 0);   // a 16-byte slot
                for (int k = 0; k < kDerivLane; k++)
                    put(derivative_stage_index(u0 + k, c0), u0 + k);
            }
        }
        put(derivative_stage_index(c0 - 1, c0), derivative_left(c0));
        put(derivative_stage_index(end, c0), end < U ? end : U - 1);
        for (int tid = 0; tid < kDerivBlock; tid++) {
            const int u0 = c0 + kDerivLane * tid;
            if (u0 >= end)
                continue;
            groups++;
            if (u0 < U) {   // the column before the group
                const int index = derivative_stage_index(derivative_left(u0), c0);
                CHECK(index >= 0 && index < kDerivStage && stage[(size_t)index] == derivative_left(u0));
            }
            if (u0 + kDerivLane < U) {   // the column after it
                const int index = derivative_stage_index(u0 + kDerivLane, c0);
                CHECK(index >= 0 && index < kDerivStage && stage[(size_t)index] == u0 + kDerivLane);
            }
            for (int k = 0; k < kDerivLane * kDerivativeChannels; k++)
                out[kDerivativeChannels * u0 + k]++;
            if (!pitch)
                CHECK(u0 + kDerivLane <= U);   // raw form: a group never reaches beyond the row
        }
        if (t == 0)
            for (int k = 0; k < derivative_peeled(r); k++) {
                const int u = derivative_peeled_column(r, k);
                CHECK(u >= 0 && u < U && (u < r.head || u >= r.head + r.body));
                for (int c = 0; c < kDerivativeChannels; c++)
                    out[kDerivativeChannels * u + c]++;
            }
    }
    for (size_t i = 0; i < written.size(); i++)
        CHECK(written[i] == 1);
    return groups;
}

int main()
{
    CHECK(kDerivTile == 1024 && kDerivStage >= kDerivTile + kDerivLane + 1 && kDerivBlock % 64 == 0);
    const int wide[] = {1019, 1020, 1021, 1023, 1024, 1025, 1027, 1028, 2047, 2049, 4100};
    std::vector<int> widths;
    for (int U = 1; U <= 300; U++)
        widths.push_back(U);
    for (int U : wide)
        widths.push_back(U);
    long long groups = 0;
    for (int U : widths)
        for (int V = 1; V <= 3; V++)
            for (int S = 1; S <= 2; S++) {
                const int pitch = (U + 1 + 63) / 64 * 64;   // plan::volume_pitch
                groups += walk(V * S, U, pitch, true);
                groups += walk(V * S, U, 0, true);
                groups += walk(V * S, U, 0, false);
            }
    CHECK(groups > 0);
    // rows of every alignment in one field: U = 7, four rows start at 0, 7, 14, 21 floats
    for (int row = 0; row < 4; row++) {
        const DerivativeRow r = derivative_row_raw((long long)row * 7, 7, true);
        CHECK(r.head == (4 - row * 7 % 4) % 4 && r.body == 4 && r.head + r.body + r.tail == 7);
    }
    CHECK(derivative_row_raw(1, 2, true).head == 2 && derivative_row_raw(1, 2, true).body == 0);   // a row shorter than its lead
    CHECK(derivative_row_raw(0, 9, false).head == 9 && derivative_peeled(derivative_row_raw(0, 9, false)) == 9);
    CHECK(derivative_row_raw(((long long)1 << 40) + 3, 6, true).head == 1);

    // the weights, the option, the cap
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(derivative_weight_ok(1.0f) && derivative_weight_ok(1e-30f) && derivative_weight_ok(3e38f));
    CHECK(!derivative_weight_ok(0.0f) && !derivative_weight_ok(-1.0f) && !derivative_weight_ok(inf) && !derivative_weight_ok(-inf) &&
          !derivative_weight_ok(nan));
    CHECK(derivative_option_ok(0.0f) && derivative_option_ok(2.0f) && !derivative_option_ok(-0.5f) && !derivative_option_ok(inf) &&
          !derivative_option_ok(nan));
    CHECK(derivative_hi_ok(0.0f) && derivative_hi_ok(1.0f) && derivative_hi_ok(inf) && !derivative_hi_ok(-1.0f) && !derivative_hi_ok(nan));
    CHECK(derivative_hi_f32(-2.0f) == 0.0f && derivative_hi_f32(0.75f) == 0.75f && derivative_hi_int(1) == 255.0f && derivative_hi_int(2) == 65535.0f);
    CHECK(derivative_half_weight(3.0f) == 1.5f);
    // the rule's rounding of integer elements: ties to even
    CHECK(derivative_feature<true>(1.0f, 0.0f, 0.5f, 255.0f) == 0.0f && derivative_feature<true>(3.0f, 0.0f, 0.5f, 255.0f) == 2.0f &&
          derivative_feature<true>(0.0f, 5.0f, 0.5f, 255.0f) == 2.0f && derivative_feature<true>(255.0f, 0.0f, 4.0f, 255.0f) == 255.0f);
    CHECK(derivative_feature<false>(1.0f, 0.0f, 0.5f, 1.0f) == 0.5f && derivative_feature<false>(0.0f, 1.0f, 4.0f, 1.0f) == 1.0f);

    // shapes
    CHECK(derivative_shape(1, 1, 1) == kDerivOk && derivative_shape(0, 1, 1) == kDerivBadShape && derivative_shape(1, -1, 1) == kDerivBadShape &&
          derivative_shape(1, 1, 0) == kDerivBadShape);
    CHECK(derivative_shape(1, 1, INT_MAX / 3 + 1) == kDerivTooLarge && derivative_shape(65536, 65536, 4) == kDerivTooLarge);
    CHECK(derivative_grid(0) == 0 && derivative_grid(5) == 5 && derivative_grid(1 << 20) == kDerivGridCap);
    CHECK(derivative_bytes(10, 30) == 160);
    std::printf("derivative plan tests ok (%lld groups)\n", groups);
    return 0;
}
