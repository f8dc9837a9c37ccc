// What the library compiles of the depth scan (K2), read from the headers it is built from: the register kernels' slot
// counts (RSLF_SPAD_LIST_*), the on-chip kernel's ladder per translation unit (RSLF_CHIP_LADDER_*), and the resident
// prefixes the streaming kernels can be asked for (stream_resident_for / stream_px_resident_for, k2_stream.hpp).  Then,
// for each "S C" pair read from stdin, the kernel choice the plan makes for that volume.  Host code only: built by
// tests/test_scan_coverage_cpu.py with hipcc --cuda-host-only (the stream prefixes live in a device header).
#include <cstdio>
#include <set>

#include "k2_reg.hpp"
#include "k2_stream.hpp"
#include "rslf_plan.hpp"

using namespace rslf;

static void stream_prefixes(int C)
{
    std::set<int> row, px;
    for (int S = 1; (size_t)plan::kScanWavesPerTile * S * sizeof(float) <= plan::kScanOffsetTableBytes; S++) {
        row.insert(stream_resident_for(S, C));
        px.insert(stream_px_resident_for(S, C));
    }
    for (int n : row)
        std::printf("nres %d row %d\n", C, n);
    for (int n : px)
        std::printf("nres %d px %d\n", C, n);
}

int main()
{
#define SPAD_1(N) std::printf("spad 1 %d %d %d %d %d %d\n", N, scan_reg_waves(N, 1), (int)scan_reg_best_in_lds(N, 1), (int)scan_reg_trim(N, 1), (int)packed_long_unit(N, 1), (int)scan_reg_tap_table(N, 1));
#define SPAD_3(N) std::printf("spad 3 %d %d %d %d %d %d\n", N, scan_reg_waves(N, 3), (int)scan_reg_best_in_lds(N, 3), (int)scan_reg_trim(N, 3), (int)packed_long_unit(N, 3), (int)scan_reg_tap_table(N, 3));
    RSLF_SPAD_LIST_1CH(SPAD_1)
    RSLF_SPAD_LIST_3CH(SPAD_3)
#undef SPAD_1
#undef SPAD_3
#define RUNG_A(NA, NL) std::printf("rung A %d %d %d\n", NA, NL, plan::ChipRung{NA, NL}.views());
#define RUNG_B(NA, NL) std::printf("rung B %d %d %d\n", NA, NL, plan::ChipRung{NA, NL}.views());
#define RUNG_C(NA, NL) std::printf("rung C %d %d %d\n", NA, NL, plan::ChipRung{NA, NL}.views());
    RSLF_CHIP_LADDER_A(RUNG_A)
    RSLF_CHIP_LADDER_B(RUNG_B)
    RSLF_CHIP_LADDER_C(RUNG_C)
#undef RUNG_A
#undef RUNG_B
#undef RUNG_C
    for (int i = 0; i < plan::kChipRungs; i++)
        std::printf("ladder %d %d\n", i, plan::kChipLadder[i].views());
    std::printf("chip top %d max %d first %d min %d padmax %d\n", plan::kChipTopS, plan::kChipMaxS, RSLF_CHIP_FIRST_S, plan::kChipMinS,
                plan::kChipPadMax);
    stream_prefixes(1);
    stream_prefixes(3);
    int S = 0, C = 0;
    while (std::scanf("%d %d", &S, &C) == 2)
        std::printf("case %d %d spad %d rung %d chip %d nres %d nres_px %d\n", S, C, plan::pick_spad(S, C), plan::chip_rung_for(S),
                    (int)plan::chip_takes(S, C), stream_resident_for(S, C), stream_px_resident_for(S, C));
    return 0;
}
