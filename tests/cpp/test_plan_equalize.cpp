// The plan of the per-view equalisation (csrc/rslf_plan_equalize.hpp) on the CPU, under AddressSanitizer / UBSan: both
// kernels' walks of k19_equalize.hpp re-enacted from the plan's functions over every U in 1..300 and eleven wide rows, V in
// 1..3, S in 1..5, C in {1, 3}, the volume form and the dense form from an aligned and an unaligned base.
//   statistics: every float < U * C of every row is counted exactly once, by a workgroup that is walking that row's view; no
//               pad float is counted; every 16-byte load lies inside its row and is 16-byte aligned;
//   apply:      every float of every row, pad included in the volume form, is written exactly once; every 16-byte store lies
//               inside its row;
//   both:       a lane's float j has the channel the plan says, and the grids keep their cap.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rslf_plan_equalize.hpp"

using namespace rslf;
using namespace rslf::plan;

#define CHECK(cond)                                                                         \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            std::fprintf(stderr, "%s:%d: %s\n  V=%d S=%d U=%d C=%d form=%d\n", __FILE__, __LINE__, #cond, g_V, g_S, g_U, g_C, g_form); \
            std::exit(1);                                                                   \
        }                                                                                   \
    } while (0)

static int g_V, g_S, g_U, g_C, g_form;

enum Form { kVolume = 0, kDenseAligned = 1, kDenseUnaligned = 2 };

static int volume_pitch(int U) { return (U + 1 + 63) / 64 * 64; }   // (plan::volume_pitch: beyond U, a multiple of 64)

static EqualizeRow row_of(Form form, int pitch, long long row, int U)
{
    return form == kVolume ? equalize_row_volume(pitch) : equalize_row_dense(row * U, U, form == kDenseAligned);
}

// One lane group or one peeled pixel lands in `hits`; loads is bumped per 16-byte access.
struct Walk {
    int C, U, row_px;
    Form form;
    std::vector<std::vector<int> > hits;   // [row][float of the row]
    long long vector_accesses = 0;
};

static void group(Walk& w, long long row, int p0, bool count_pad)
{
    const int C = w.C;
    // the group's 4 C floats lie inside the row, as C accesses of 16 bytes at multiples of 16 bytes from an aligned base
    CHECK(p0 >= 0 && (long long)(p0 + kEqLane) * C <= (long long)w.row_px * C);
    CHECK(w.form != kDenseUnaligned);   // an unaligned base has no body
    CHECK(((row * w.row_px + p0) * C) % 4 == 0);
    w.vector_accesses += C;
    for (int j = 0; j < kEqLane * C; j++) {
        const int px = p0 + equalize_float_pixel(j, C), c = equalize_float_channel(j, C);
        const int f = p0 * C + j;                  // the float the register holds
        CHECK(f == px * C + c && c == f % C && c >= 0 && c < C);
        if (px < w.U || count_pad)
            w.hits[(size_t)row][(size_t)f]++;
    }
}

static void peel(Walk& w, long long row, const EqualizeRow& r)
{
    for (int k = 0; k < equalize_peeled(r); k++) {
        const int p = equalize_peeled_pixel(r, k);
        CHECK(p >= 0 && p < w.U);
        for (int c = 0; c < w.C; c++)
            w.hits[(size_t)row][(size_t)p * w.C + c]++;
    }
}

static void one(int V, int S, int U, int C, Form form)
{
    g_V = V, g_S = S, g_U = U, g_C = C, g_form = form;
    CHECK(equalize_shape(V, S, U, C) == kEqOk);
    const int pitch = form == kVolume ? volume_pitch(U) : 0;
    const int row_px = pitch ? pitch : U;
    const long long rows = (long long)V * S;
    for (long long row = 0; row < rows; row++) {
        const EqualizeRow r = row_of(form, pitch, row, U);
        CHECK(r.head >= 0 && r.body >= 0 && r.tail >= 0 && r.head + r.body + r.tail == row_px && r.body % kEqLane == 0);
        CHECK(r.head < kEqLane || form == kDenseUnaligned);
        CHECK(r.tail < kEqLane || form == kDenseUnaligned);
    }
    // ---- the statistics kernel ----
    {
        Walk w = {C, U, row_px, form, std::vector<std::vector<int> >((size_t)rows, std::vector<int>((size_t)row_px * C, 0))};
        const int tpr = equalize_tiles_per_row(U);
        const EqualizeStatsGrid g = equalize_stats_grid(V, S, tpr);
        const unsigned blocks = equalize_stats_blocks(g);
        CHECK(g.per_view >= 1 && g.groups >= 1 && blocks <= kEqGridCap && blocks >= 1);
        CHECK(g.groups <= S && (S > (int)kEqGridCap || g.groups == S));
        const long long items = (long long)V * tpr;
        CHECK(g.per_view <= items);
        std::vector<int> atomics((size_t)S, 0);   // workgroups that add a view's totals
        for (unsigned b = 0; b < blocks; b++) {
            const int member = equalize_stats_member(g, b);
            CHECK(member >= 0 && member < g.per_view);
            for (int s = equalize_stats_team(g, b); s < S; s += g.groups) {
                atomics[(size_t)s]++;
                for (long long i = member; i < items; i += g.per_view) {
                    const int v = (int)(i / tpr), t = (int)(i - (long long)v * tpr);
                    const long long row = (long long)v * S + s;
                    CHECK(v < V && row % S == s);
                    const EqualizeRow r = row_of(form, pitch, row, U);
                    if (!equalize_tile_works(r, t))
                        continue;
                    for (int tid = 0; tid < kEqBlock; tid++) {
                        const int p0 = equalize_lane_first(r, t, tid);
                        if (!equalize_lane_works(r, p0))
                            break;   // (p0 grows with tid)
                        if (p0 < U)
                            group(w, row, p0, false);
                    }
                    if (t == 0)
                        peel(w, row, r);
                }
            }
        }
        for (int s = 0; s < S; s++)
            CHECK(atomics[(size_t)s] == g.per_view);   // one add per total, workgroup and view
        for (long long row = 0; row < rows; row++)
            for (int f = 0; f < row_px * C; f++)
                CHECK(w.hits[(size_t)row][(size_t)f] == (f < U * C ? 1 : 0));
    }
    // ---- the apply kernel ----
    {
        Walk w = {C, U, row_px, form, std::vector<std::vector<int> >((size_t)rows, std::vector<int>((size_t)row_px * C, 0))};
        const int tpr = equalize_tiles_per_row(row_px);
        const long long tiles = rows * tpr;
        const unsigned grid = equalize_apply_grid(tiles);
        CHECK(grid >= 1 && grid <= kEqGridCap && (long long)grid <= tiles);
        for (unsigned b = 0; b < grid; b++)
            for (long long tile = b; tile < tiles; tile += grid) {
                const long long row = tile / tpr;
                const int t = (int)(tile - row * tpr);
                const EqualizeRow r = row_of(form, pitch, row, U);
                if (!equalize_tile_works(r, t))
                    continue;
                for (int tid = 0; tid < kEqBlock; tid++) {
                    const int p0 = equalize_lane_first(r, t, tid);
                    if (!equalize_lane_works(r, p0))
                        break;
                    group(w, row, p0, true);
                }
                if (t == 0)
                    peel(w, row, r);
            }
        for (long long row = 0; row < rows; row++)
            for (int f = 0; f < row_px * C; f++)
                CHECK(w.hits[(size_t)row][(size_t)f] == 1);
        if (form == kDenseUnaligned)
            CHECK(w.vector_accesses == 0);
    }
}

int main()
{
    static const int wide[11] = {1023, 1024, 1025, 1027, 2047, 2048, 2049, 3001, 4096, 4099, 10001};
    long long configs = 0;
    for (int C = 1; C <= 3; C += 2)
        for (int form = kVolume; form <= kDenseUnaligned; form++)
            for (int V = 1; V <= 3; V++)
                for (int S = 1; S <= 5; S++) {
                    for (int U = 1; U <= 300; U++, configs++)
                        one(V, S, U, C, (Form)form);
                    for (int k = 0; k < 11; k++, configs++)
                        one(V, S, wide[k], C, (Form)form);
                }
    // the grids at their caps: more views than the cap, more rows than the cap
    one(1, 2100, 3, 1, kDenseAligned);
    one(2, 2100, 5, 3, kVolume);
    one(700, 3, 6, 1, kDenseAligned);
    one(1100, 2, 2050, 3, kDenseAligned);
    // the refusals of a shape
    g_V = g_S = g_U = g_C = g_form = 0;
    CHECK(equalize_shape(0, 1, 1, 1) == kEqBadShape && equalize_shape(1, 0, 1, 1) == kEqBadShape && equalize_shape(1, 1, 0, 1) == kEqBadShape);
    CHECK(equalize_shape(1, 1, 1, 2) == kEqBadShape && equalize_shape(1, 1, 1, 4) == kEqBadShape);
    CHECK(equalize_shape(46341, 1, 46341, 1) == kEqTooLarge);            // V * U = 2^31 + 4 * 46341 + ...: beyond 2^31 - 1
    CHECK(equalize_shape(46340, 1, 46341, 3) == kEqOk);                  // 2147441940 samples
    CHECK(equalize_shape(1, 1, 2147483647, 1) == kEqTooLarge);           // 3 * U does not fit an int
    CHECK(equalize_shape(1, 1, (INT_MAX - 64) / 3, 3) == kEqOk);
    CHECK(equalize_shape(65536, 65536, 1, 1) == kEqTooLarge);            // V * S rows
    CHECK(eq_mode_ok(RSLF_EQ_MODE_GAIN) && eq_mode_ok(RSLF_EQ_MODE_AFFINE) && !eq_mode_ok(0) && !eq_mode_ok(3));
    CHECK(eq_max_gain_ok(1.0f) && eq_max_gain_ok(4.0f) && !eq_max_gain_ok(0.5f) && !eq_max_gain_ok(INFINITY) && !eq_max_gain_ok(NAN));
    CHECK(eq_hi_ok(1.0f) && !eq_hi_ok(0.0f) && !eq_hi_ok(-1.0f) && !eq_hi_ok(INFINITY) && !eq_hi_ok(NAN));
    std::printf("equalize plan tests ok (%lld configurations)\n", configs);
    return 0;
}
