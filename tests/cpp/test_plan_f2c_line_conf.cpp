// Where a level of the fine-to-coarse pyramid reads its validity from (rslf_plan.hpp: f2c_validity) and the pyramid sizes the
// level outputs are laid out by, compiled with g++ alone and run under AddressSanitizer / UBSan
// (tests/test_f2c_line_conf_cpu.py).
#include <cstdio>
#include <cstdlib>

#include "rslf_plan.hpp"

using namespace rslf::plan;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

int main()
{
    // dc.hpp:893-915: accept_all comes first, whatever the mode and the C_d switch
    for (int mode = 0; mode <= 2; mode++)
        for (int disp = 0; disp <= 1; disp++)
            CHECK(f2c_validity(true, disp != 0, mode) == kValidAll);
    // C_l in the gating mode alone, and only where C_d does not come first in the #ifdef chain
    CHECK(f2c_validity(false, false, kLineConfGate) == kValidLineConf);
    CHECK(f2c_validity(false, true, kLineConfGate) == kValidEdgeConf);
    // the default build and what the macro compiles to: C_e
    CHECK(f2c_validity(false, false, kLineConfOff) == kValidEdgeConf);
    CHECK(f2c_validity(false, true, kLineConfOff) == kValidEdgeConf);
    CHECK(f2c_validity(false, false, kLineConfAsBuilt) == kValidEdgeConf);
    CHECK(f2c_validity(false, true, kLineConfAsBuilt) == kValidEdgeConf);
    // the validity follows the sweep's gate: the two never read different line planes
    for (int mode = 0; mode <= 2; mode++)
        for (int disp = 0; disp <= 1; disp++)
            CHECK((f2c_validity(false, disp != 0, mode) == kValidLineConf) == (sweep_gate(disp != 0, mode) == kGateLineConf));

    // the level sizes the per-level outputs are sized by
    const std::vector<LevelDims> a = f2c_pyramid(44, 64, -1);
    CHECK(a.size() == 3 && a[0].V == 44 && a[0].U == 64 && a[1].V == 22 && a[1].U == 32 && a[2].V == 11 && a[2].U == 16);
    const std::vector<LevelDims> c = f2c_pyramid(90, 130, -1);
    CHECK(c.size() == 4 && c[1].V == 45 && c[1].U == 65 && c[2].V == 22 && c[2].U == 32 && c[3].V == 11 && c[3].U == 16);
    CHECK(f2c_pyramid(90, 130, 2).size() == 2);
    CHECK(f2c_pyramid(10, 130, -1).empty());

    std::printf("fine-to-coarse line confidence plan tests ok\n");
    return 0;
}
