// Host-side decisions of the score rows (rslf_plan.hpp, "score rows"): which kernel serves a request, the sink's run length
// and LDS, the launches of a window of scanlines, the offsets into the output and the passes of the host form.
// Built with g++ under AddressSanitizer + UBSan and run directly (tests/test_plan_scores_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rslf_plan.hpp"

using namespace rslf;
using namespace rslf::plan;

static int g_checks = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        g_checks++;                                                             \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

static void test_kernel_choice()
{
    for (int C = 1; C <= 3; C += 2)
        for (int S = 1; S <= 260; S++)
            for (int in_range = 0; in_range < 2; in_range++)
                for (int linear = 0; linear < 2; linear++)
                    for (int force = 0; force <= 2; force++) {
                        int spad = -1;
                        const int kind = choose_score_kernel(S, C, in_range != 0, linear != 0, force, &spad);
                        const bool reg = pick_spad(S, C) != 0 && in_range && linear && force == 0;
                        CHECK(kind == (reg ? RSLF_SCAN_REG : RSLF_SCAN_GENERIC));
                        CHECK(spad == (reg ? pick_spad(S, C) : 0));
                        if (reg)
                            CHECK(spad >= S && spad % 8 == 0);
                    }
    // the table's cases: slot counts and the generic form's stream-class view counts
    int spad = 0;
    CHECK(choose_score_kernel(101, 1, true, true, 0, &spad) == RSLF_SCAN_REG && spad == 104);
    CHECK(choose_score_kernel(9, 1, true, true, 0, &spad) == RSLF_SCAN_REG && spad == 16);
    CHECK(choose_score_kernel(104, 1, true, true, 0, &spad) == RSLF_SCAN_REG && spad == 104);
    CHECK(choose_score_kernel(180, 1, true, true, 0, &spad) == RSLF_SCAN_REG && spad == 192);
    CHECK(choose_score_kernel(17, 3, true, true, 0, &spad) == RSLF_SCAN_REG && spad == 24);
    CHECK(choose_score_kernel(44, 3, true, true, 0, &spad) == RSLF_SCAN_REG && spad == 48);
    CHECK(choose_score_kernel(200, 1, true, true, 0, &spad) == RSLF_SCAN_GENERIC && spad == 0);
    CHECK(choose_score_kernel(60, 3, true, true, 0, &spad) == RSLF_SCAN_GENERIC && spad == 0);
}

static void test_run_length_and_lds()
{
    const size_t device_lds = (size_t)160 << 10;
#define SLOTS(N) slots.push_back(N);
    for (int C = 1; C <= 3; C += 2) {
        std::vector<int> slots;
        if (C == 1) {
            RSLF_SPAD_LIST_1CH(SLOTS)
        } else {
            RSLF_SPAD_LIST_3CH(SLOTS)
        }
        slots.push_back(0);   // the generic form: no offset table
        for (int spad : slots)
            for (int table = 1; table <= 4; table += 3) {
                const int run = score_run_length(spad, C);
                CHECK(run == kScoreRun && run >= 1 && 64 % run == 0);
                const size_t lds = score_lds_bytes(spad, table);
                // the parking block [pixel][run + 1], the pixel numbers and the offset table of each of the four waves
                CHECK(lds == (size_t)kScanWavesPerTile * (64 * (size_t)(run + 1) * 4 + 64 * 4 + (size_t)spad * table * 4));
                CHECK(lds <= kScoreLdsLimit && kScoreLdsLimit <= device_lds);
                // as many workgroups per CU as the register file could ever hold waves per SIMD (C * spad sample registers
                // of 512 each, eight at most) fit the CU's LDS: the sink never lowers a kernel's occupancy
                const int waves = spad ? std::min(8, 512 / (C * spad)) : 8;
                CHECK((size_t)waves * score_lds_bytes(spad, 1) <= device_lds);
            }
    }
#undef SLOTS
    CHECK(3 * score_lds_bytes(104, 4) <= device_lds);   // the c3 kernel's three
    CHECK((kScoreRun + 1) % 2 == 1);                    // the odd pitch
}

static void test_window_plans()
{
    const int Us[] = {1, 63, 64, 65, 130, 1920, 4096};
    const int Ds[] = {2, 5, 16, 33, 256, 512};
    for (int U : Us)
        for (int D : Ds)
            for (int V : {1, 3, 128, 1080})
                for (int v_first : {0, 1, V / 2, V - 1})
                    for (int n_rows : {1, 2, V - v_first})
                        for (int force : {0, 1, 4, 64}) {
                            if (v_first < 0 || v_first >= V || n_rows < 1 || n_rows > V - v_first)
                                continue;
                            const ScanPlan p = score_plan(RSLF_SCAN_REG, 104, n_rows, U, D, 256, 3, force);
                            CHECK(p.groups >= 1 && p.groups <= 64 && !p.packed && p.px_waves == 0 && p.records == 0 && p.tickets == 0);
                            CHECK(p.tile_w == 64 && p.tiles_per_row == (U + 63) / 64 && p.rows_per_launch >= 1);
                            CHECK(p.groups == 1 || D >= 2 * kScanWavesPerTile * p.groups);
                            if (force > 0 && D >= 2 * kScanWavesPerTile * force)
                                CHECK(p.groups == force);
                            std::vector<ScanLaunch> ls;
                            long long bad = 0;
                            CHECK(score_launches(v_first, n_rows, U, p, &ls, &bad));
                            // every scanline of the window exactly once, in order; every (tile, group) of a launch within its grid
                            int next = v_first;
                            for (const ScanLaunch& l : ls) {
                                CHECK(l.v0 == next);
                                const int rows = std::min(p.rows_per_launch, v_first + n_rows - l.v0);
                                CHECK(rows >= 1 && l.logical_blocks == rows * p.tiles_per_row * p.groups);
                                CHECK((long long)l.grid >= l.logical_blocks && l.grid == (unsigned)l.per_xcd * 8);
                                next += rows;
                            }
                            CHECK(next == v_first + n_rows);
                        }
    // few tiles: groups; many: one
    CHECK(score_plan(RSLF_SCAN_REG, 104, 1, 64, 256, 256, 3, 0).groups > 1);
    CHECK(score_plan(RSLF_SCAN_REG, 104, 1080, 1920, 256, 256, 3, 0).groups == 1);
    CHECK(score_plan(RSLF_SCAN_REG, 104, 128, 1920, 256, 256, 3, 0).groups == 2);   // 3840 tiles: five rounds of 768 workgroups
    CHECK(score_plan(RSLF_SCAN_GENERIC, 0, 2, 64, 2, 256, 4, 0).groups == 1);
    // the long rows of tests/test_gpu_score_instantiations.py: the "force_groups" hook holds at 70 and 133 hypotheses, for
    // every kernel and window they run, so a wave's share is ceil(D / (4 * groups)) -- more than one run of kScoreRun
    for (int n_rows : {1, 2})
        for (int spad : {0, 16, 24, 104}) {
            const int kind = spad ? RSLF_SCAN_REG : RSLF_SCAN_GENERIC, waves = spad == 104 ? 3 : spad == 16 ? 7 : 4;
            CHECK(score_plan(kind, spad, n_rows, 300, 70, 256, waves, 1).groups == 1);
            CHECK(score_plan(kind, spad, n_rows, 300, 133, 256, waves, 1).groups == 1);
            CHECK(score_plan(kind, spad, n_rows, 300, 133, 256, waves, 2).groups == 2);
            CHECK(score_plan(kind, spad, n_rows, 300, 70, 256, waves, 2).groups == 2);
            CHECK(score_plan(kind, spad, n_rows, 300, 70, 256, waves, 0).groups == 8);     // left alone: waves of 3, no full run
            CHECK(score_plan(kind, spad, n_rows, 300, 133, 256, waves, 0).groups == 16);   // ... of 3
        }
    CHECK((70 + 3) / 4 == 18 && 70 - 3 * 18 == kScoreRun);                // waves of 18, 18, 18 and one of exactly a run
    CHECK((133 + 3) / 4 == 34 && 34 > 2 * kScoreRun && 133 - 3 * 34 == 31);
    CHECK((133 + 7) / 8 == 17 && 17 == kScoreRun + 1 && 133 - 7 * 17 == 14);
    // the table's own rows (300 pixels, 24 hypotheses) run in two groups: waves of 3
    CHECK(score_plan(RSLF_SCAN_REG, 104, 1, 300, 24, 256, 3, 0).groups == 2);
    // a window too large for one grid goes in several launches
    {
        const ScanPlan p = score_plan(RSLF_SCAN_GENERIC, 0, 65535, 1 << 22, 512, 256, 4, 0);
        std::vector<ScanLaunch> ls;
        long long bad = 0;
        CHECK(score_launches(0, 65535, 1 << 22, p, &ls, &bad) && ls.size() > 1);
        long long rows = 0;
        for (const ScanLaunch& l : ls)
            rows += l.logical_blocks / (p.tiles_per_row * p.groups);
        CHECK(rows == 65535);
    }
}

static void test_offsets_and_passes()
{
    // monotone in (row, u, d), dense
    const int U = 7, D = 5;
    size_t want = 0;
    for (int r = 0; r < 3; r++)
        for (int u = 0; u < U; u++)
            for (int d = 0; d < D; d++)
                CHECK(score_offset(r, u, d, U, D) == want++);
    // c5: 4096 x 2160 x 512 floats, past 2^31
    const size_t last = score_offset(2159, 4095, 511, 4096, 512);
    CHECK(last == (size_t)4096 * 2160 * 512 - 1 && last > ((size_t)1 << 31));
    CHECK(score_offset(2159, 0, 0, 4096, 512) == (size_t)2159 * 4096 * 512);

    for (int Uw : {1, 130, 1920, 4096})
        for (int Dw : {2, 33, 256, 512})
            for (size_t budget : {(size_t)0, (size_t)1, (size_t)1 << 10, (size_t)100 << 10, (size_t)256 << 20, ~(size_t)0}) {
                const int rows = score_window_rows(Uw, Dw, budget);
                const size_t row_bytes = (size_t)Uw * Dw * 4;
                CHECK(rows >= 1);
                if (budget >= row_bytes) {
                    CHECK((size_t)rows <= budget / row_bytes);               // never over the budget when one scanline fits
                    CHECK((size_t)rows == std::min<size_t>(budget / row_bytes, INT32_MAX));
                } else {
                    CHECK(rows == 1);
                }
                // the passes tile a window
                for (int n_rows : {1, 3, 128}) {
                    const int pass = std::min(n_rows, rows);
                    int covered = 0, passes = 0;
                    for (int r0 = 0; r0 < n_rows; r0 += pass) {
                        CHECK(r0 == covered);
                        covered += std::min(pass, n_rows - r0);
                        passes++;
                    }
                    CHECK(covered == n_rows && passes == (n_rows + pass - 1) / pass);
                }
            }
    // the first GPU case through 100 KiB: 130 x 33 floats a scanline = 17 160 B, five a pass
    CHECK(score_window_rows(130, 33, (size_t)16 << 10) == 1 && score_window_rows(130, 33, (size_t)100 << 10) == 5);
}

int main()
{
    test_kernel_choice();
    test_run_length_and_lds();
    test_window_plans();
    test_offsets_and_passes();
    std::printf("plan score tests ok: %d checks\n", g_checks);
    return 0;
}
