// csrc/rslf_plan_level_dilate.hpp and csrc/k18_ranges_rule.hpp compiled alone by g++ under -fsanitize=address,undefined: the
// two K18 kernels replayed on the host, lane for lane, from the grids the plan gives.  For every U in 1..300 and f in 1..8:
// every output element of both kernels is written exactly once, every read index lies inside its row, every 16-byte store
// is aligned, and what is written is the rule's value.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rslf_plan_level_dilate.hpp"

using namespace rslf;

#define CHECK(c)                                                               \
    do {                                                                       \
        if (!(c)) {                                                            \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

// k18_dilate_ranges as the kernel walks it: grid (x, y), lanes of a workgroup, the row loop.
static void replay_ranges(int U, int f, size_t rows, bool vec, unsigned cap_y)
{
    int Ud = 0;
    CHECK(plan::dilated_width(U, f, &Ud) == plan::kDilateOk);
    const unsigned gx = plan::ranges_grid_x(Ud);
    unsigned gy = plan::ranges_grid_y(rows);
    if (cap_y && gy > cap_y)
        gy = cap_y;   // (a smaller cap than the plan's: the stride over the rows, without thousands of rows)
    CHECK(gx >= 1 && gy >= 1 && gy <= plan::kRangesRowCap);
    std::vector<float> src((size_t)rows * U);
    for (size_t k = 0; k < src.size(); k++)
        src[k] = (float)((k * 37) % 101) - 50.0f;
    std::vector<int> written((size_t)rows * Ud, 0);
    std::vector<float> out((size_t)rows * Ud, 0.0f);
    for (unsigned by = 0; by < gy; by++)
        for (unsigned bx = 0; bx < gx; bx++)
            for (int tid = 0; tid < plan::kDilateBlock; tid++) {
                const long long g = (long long)bx * plan::kDilateBlock + tid;
                for (size_t r = by; r < rows; r += gy) {
                    const int a = plan::ranges_row_offset(r, Ud, vec);
                    CHECK(a >= 0 && a < 4);
                    const RangesSpan s = ranges_span(g, a, Ud);
                    CHECK(s.count >= 0 && s.count <= 4);
                    if (!s.count)
                        continue;
                    CHECK(s.first >= 0 && s.first + s.count <= Ud);
                    if (vec && s.count == 4)
                        CHECK((r * (size_t)Ud + (size_t)s.first) % 4 == 0);   // the 16-byte store is aligned
                    for (int k = 0; k < s.count; k++) {
                        const int j = s.first + k;
                        int i, p;
                        ranges_source(j, f, &i, &p);
                        CHECK(i >= 0 && i < U && p >= 0 && p < f);
                        CHECK(p == 0 || i + 1 < U);   // the second neighbour is read only between two columns
                        written[r * (size_t)Ud + j]++;
                        out[r * (size_t)Ud + j] = ranges_lower(&src[r * (size_t)U], j, f);
                    }
                }
            }
    for (size_t k = 0; k < written.size(); k++)
        CHECK(written[k] == 1);
    for (size_t r = 0; r < rows; r++)
        for (int i = 0; i < U; i++) {
            CHECK(out[r * (size_t)Ud + (size_t)i * f] == src[r * (size_t)U + i]);
            for (int p = 1; p < f && i + 1 < U; p++) {
                const float a = src[r * (size_t)U + i], b = src[r * (size_t)U + i + 1];
                CHECK(out[r * (size_t)Ud + (size_t)i * f + p] == (a < b ? a : b));
            }
        }
    // the groups of a row never exceed what grid.x holds
    for (int a = 0; a < 4; a++)
        CHECK(ranges_groups(a, Ud) <= (long long)gx * plan::kDilateBlock);
}

// k18_undilate_many: grid (x, y, z); lane u of plane z copies in[r][u * f] for its rows.
static void replay_undilate(int U, int f, size_t rows, int n4, int n1, unsigned cap_y)
{
    int Ud = 0;
    CHECK(plan::dilated_width(U, f, &Ud) == plan::kDilateOk);
    CHECK(plan::undilated_width(Ud, f) == U);
    CHECK(plan::undilate_many_counts_ok(n4, n1));
    const unsigned gx = plan::undilate_grid_x(U), gz = plan::undilate_many_grid_z(n4, n1);
    unsigned gy = plan::undilate_grid_y(rows);
    if (cap_y && gy > cap_y)
        gy = cap_y;
    CHECK(gx >= 1 && gy >= 1 && gz == (unsigned)(n4 + n1) && gz <= 65535u);
    std::vector<int> written((size_t)gz * rows * U, 0);
    for (unsigned bz = 0; bz < gz; bz++)
        for (unsigned by = 0; by < gy; by++)
            for (unsigned bx = 0; bx < gx; bx++)
                for (int tid = 0; tid < plan::kDilateBlock; tid++) {
                    const int u = (int)(bx * plan::kDilateBlock + tid);
                    if (u >= U)
                        continue;
                    const size_t col = (size_t)u * f;
                    CHECK(col < (size_t)Ud);   // the read stays inside the dilated row
                    for (size_t r = by; r < rows; r += gy)
                        written[((size_t)bz * rows + r) * U + u]++;
                }
    for (size_t k = 0; k < written.size(); k++)
        CHECK(written[k] == 1);
}

int main()
{
    for (int U = 1; U <= 300; U++)
        for (int f = 1; f <= 8; f++) {
            const size_t rows = 1 + (size_t)((U + f) % 5);
            replay_ranges(U, f, rows, true, 0);
            replay_ranges(U, f, rows, false, 0);
            replay_ranges(U, f, 7, true, 3);    // rows strided over a capped grid.y
            replay_undilate(U, f, rows, 1 + (U % 8), U % 3, 0);
            replay_undilate(U, f, 7, 7, 0, 3);
        }
    // the counts one launch serves
    CHECK(!plan::undilate_many_counts_ok(0, 0) && !plan::undilate_many_counts_ok(9, 0) && !plan::undilate_many_counts_ok(1, 3));
    CHECK(plan::undilate_many_counts_ok(8, 2) && plan::undilate_many_counts_ok(0, 1));
    CHECK(plan::ranges_grid_y(0) == 0 && plan::ranges_grid_y(100000) == plan::kRangesRowCap && plan::ranges_grid_x(0) == 0);
    // 16-byte stores only when both planes start on a boundary
    alignas(16) static float buf[8];
    CHECK(plan::ranges_vector_stores(buf, buf + 4) && !plan::ranges_vector_stores(buf, buf + 1) && !plan::ranges_vector_stores(buf + 2, buf + 4));
    CHECK(plan::ranges_row_offset(3, 5, true) == 3 && plan::ranges_row_offset(3, 5, false) == 0);
    printf("level dilate plan tests ok\n");
    return 0;
}
