// What the library compiles of the score rows (k2_scores.hpp, rslf_scores.hip), read from the headers it is built from: one
// k2_score_rows_reg per slot count of RSLF_SPAD_LIST_*, with score_rows_trim, score_rows_tap_table and the scan's own
// scan_reg_trim of each taken from the constexpr functions themselves.  Then, for each line read from stdin:
//   "kernel S C force_scan"                       -> the form and slot count plan::choose_score_kernel picks
//   "plan kind spad C n_rows U dim_d force_groups" -> the hypothesis groups plan::score_plan settles on (256 CUs)
// Runs on the host and touches no device: built by tests/test_score_coverage_cpu.py with hipcc for gfx950 (k2_scores.hpp holds a
// kernel that is no template, k_score_lists, so a host-only build has no code object to link against).
#include <cstdio>
#include <cstring>

#include "k2_scores.hpp"
#include "rslf_plan.hpp"

using namespace rslf;

int main()
{
#define CELL_1(N) std::printf("cell 1 %d trim %d taps %d scan_trim %d waves %d\n", N, (int)score_rows_trim(N, 1), (int)score_rows_tap_table(N, 1), (int)scan_reg_trim(N, 1), scan_reg_waves(N, 1));
#define CELL_3(N) std::printf("cell 3 %d trim %d taps %d scan_trim %d waves %d\n", N, (int)score_rows_trim(N, 3), (int)score_rows_tap_table(N, 3), (int)scan_reg_trim(N, 3), scan_reg_waves(N, 3));
    RSLF_SPAD_LIST_1CH(CELL_1)
    RSLF_SPAD_LIST_3CH(CELL_3)
#undef CELL_1
#undef CELL_3
    std::printf("run %d waves %d\n", kScoreRun, plan::kScanWavesPerTile);
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (std::strcmp(what, "kernel") == 0) {
            int S = 0, C = 0, force = 0, spad = -1;
            if (std::scanf("%d %d %d", &S, &C, &force) != 3)
                return 1;
            const int kind = plan::choose_score_kernel(S, C, true, true, force, &spad);
            std::printf("kernel %d %d %d kind %d spad %d\n", S, C, force, kind, spad);
        } else if (std::strcmp(what, "plan") == 0) {
            int kind = 0, spad = 0, C = 0, n_rows = 0, U = 0, D = 0, force = 0;
            if (std::scanf("%d %d %d %d %d %d %d", &kind, &spad, &C, &n_rows, &U, &D, &force) != 7)
                return 1;
            const plan::ScanPlan p = plan::score_plan(kind, spad, n_rows, U, D, 256, spad ? scan_reg_waves(spad, C) : 4, force);
            std::printf("plan %d %d %d %d %d %d %d groups %d tile_w %d\n", kind, spad, C, n_rows, U, D, force, p.groups, p.tile_w);
        } else {
            return 1;
        }
    }
    return 0;
}
