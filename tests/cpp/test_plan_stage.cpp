// Host test of the output stage's layout (rslf_plan_stage.hpp) against the totals the operations promise
// (rslf_plan_consistency.hpp: consistency_out_bytes_per_cell).  Stand-alone: built by tests/test_stage_cpu.py with
// g++ -fsanitize=address,undefined.  No HIP.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "rslf_plan_consistency.hpp"
#include "rslf_plan_stage.hpp"

using namespace rslf::plan;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

static const size_t kUntouched = 0xABCDEF;

// align = 1 with the consistency check's plane order -- seen, agree, above, below, fused, then the byte plane: packed, the
// total the plan promises, for every choice of planes.
static void packed_is_the_consistency_layout(size_t n)
{
    const size_t bytes[6] = {n * 4, n * 4, n * 4, n * 4, n * 4, n};
    for (int m = 0; m < 64; m++) {
        bool wanted[6];
        int counts = 0;
        for (int i = 0; i < 6; i++) {
            wanted[i] = (m >> i & 1) != 0;
            counts += i < 4 && wanted[i];
        }
        size_t off[6] = {kUntouched, kUntouched, kUntouched, kUntouched, kUntouched, kUntouched};
        const size_t total = stage_layout(bytes, wanted, 6, 1, off);
        CHECK(total == n * consistency_out_bytes_per_cell(counts, wanted[4], wanted[5]));
        size_t at = 0;
        for (int i = 0; i < 6; i++) {
            CHECK(off[i] == (wanted[i] ? at : kUntouched));   // increasing, no padding, the others left alone
            at += wanted[i] ? bytes[i] : 0;
        }
        CHECK(at == total);
    }
}

static size_t up(size_t b, size_t align) { return (b + align - 1) / align * align; }

// align = 16 with the warp's nine planes of T = 1 target on V x U cells and C channels (rslf_warp.hip), and the novel view's
// seven: every offset a multiple of 16, unwanted planes take no room, the total the sum of the rounded sizes.
static void aligned(size_t n, size_t rows, size_t C)
{
    const size_t warp[9] = {n, n * 4, n * 4, n * 4, n * 4, n * 4 * C, n * 4, rows * 8, rows * 4};
    const size_t novel[7] = {n * 4 * C, n * 4, n, n * 4, n * 4, rows * 8, rows * 4};
    for (int which = 0; which < 2; which++) {
        const size_t* bytes = which ? novel : warp;
        const int count = which ? 7 : 9;
        for (int m = 0; m < (1 << count); m++) {
            bool wanted[9];
            size_t off[9], sum = 0;
            for (int i = 0; i < count; i++)
                wanted[i] = (m >> i & 1) != 0, off[i] = kUntouched;
            const size_t total = stage_layout(bytes, wanted, count, 16, off);
            for (int i = 0; i < count; i++) {
                CHECK(off[i] == (wanted[i] ? sum : kUntouched));
                CHECK(!wanted[i] || off[i] % 16 == 0);
                sum += wanted[i] ? up(bytes[i], 16) : 0;
            }
            CHECK(total == sum && total % 16 == 0);
        }
    }
}

static void edges()
{
    const size_t bytes[3] = {5, 0, 33};
    const bool none[3] = {false, false, false}, all[3] = {true, true, true};
    size_t off[3] = {kUntouched, kUntouched, kUntouched};
    CHECK(stage_layout(bytes, none, 3, 16, off) == 0 && stage_layout(bytes, none, 3, 1, off) == 0 && stage_layout(bytes, all, 0, 16, off) == 0);
    CHECK(off[0] == kUntouched && off[1] == kUntouched && off[2] == kUntouched);
    CHECK(stage_layout(bytes, all, 3, 16, off) == 64 && off[0] == 0 && off[1] == 16 && off[2] == 16);   // an empty plane takes no room
    CHECK(stage_layout(bytes, all, 3, 1, off) == 38 && off[0] == 0 && off[1] == 5 && off[2] == 5);
    // sizes no address space holds: refused by the one value no layout has, never wrapped
    const size_t half = SIZE_MAX / 2;
    const size_t big[3] = {half, half, 16};
    const bool two[3] = {true, true, false};
    CHECK(stage_layout(big, two, 3, 1, off) == SIZE_MAX - 1 && off[1] == half);   // the largest total there is
    CHECK(stage_layout(big, all, 3, 1, off) == kStageTooLarge);
    CHECK(stage_layout(big, two, 3, 16, off) == kStageTooLarge);   // half rounds up to half + 1: twice that wraps
    const size_t top[1] = {SIZE_MAX - 3};
    CHECK(stage_layout(top, all, 1, 1, off) == SIZE_MAX - 3 && stage_layout(top, all, 1, 16, off) == kStageTooLarge);
    const size_t max[1] = {SIZE_MAX};
    CHECK(stage_layout(max, all, 1, 1, off) == kStageTooLarge && stage_layout(max, none, 1, 16, off) == 0);
}

int main()
{
    const size_t cells[3] = {3 * 37, 3 * 40, 1}, channels[3] = {0, 1, 3};
    for (size_t n : cells) {
        packed_is_the_consistency_layout(n);
        for (size_t C : channels)
            aligned(n, n == 1 ? 1 : 3, C);
    }
    edges();
    printf("stage plan tests ok\n");
    return 0;
}
