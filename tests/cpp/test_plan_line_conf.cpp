// The host-side decisions of the sweep's line confidence (rslf_plan.hpp: modes, launches per visit, scratch sizes, the
// gate of the propagation), compiled with g++ alone and run under AddressSanitizer / UBSan (tests/test_line_conf_cpu.py).
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
    // the modes are the header's
    CHECK(kLineConfOff == RSLF_LINE_CONF_OFF && kLineConfAsBuilt == RSLF_LINE_CONF_AS_BUILT && kLineConfGate == RSLF_LINE_CONF_GATE);
    CHECK(!line_conf_mode_ok(-1) && line_conf_mode_ok(0) && line_conf_mode_ok(1) && line_conf_mode_ok(2) && !line_conf_mode_ok(3));

    // launches of a visit's finish step: today's two without line confidence, K7 with it, the median alone before K7
    // where the claims wait for C_l
    CHECK(line_conf_finish_launches(false, kLineConfOff) == 2 && line_conf_finish_launches(true, kLineConfOff) == 2);
    CHECK(line_conf_finish_launches(false, kLineConfAsBuilt) == 3 && line_conf_finish_launches(true, kLineConfAsBuilt) == 3);
    CHECK(line_conf_finish_launches(false, kLineConfGate) == 4);
    CHECK(line_conf_finish_launches(true, kLineConfGate) == 3);   // C_d gates: the claims do not wait for C_l
    CHECK(line_conf_before_claims(false, kLineConfGate) && !line_conf_before_claims(true, kLineConfGate));
    CHECK(!line_conf_before_claims(false, kLineConfAsBuilt) && !line_conf_before_claims(false, kLineConfOff));

    // scratch: nothing when off; V * S * U floats and V * U indices otherwise, in size_t (c3: 838 MB, past 2^31 at c5)
    CHECK(line_conf_columns_bytes(kLineConfOff, 540, 101, 960) == 0);
    CHECK(line_conf_argmax_bytes(kLineConfOff, 540, 960) == 0);
    CHECK(line_conf_columns_bytes(kLineConfAsBuilt, 2160, 101, 960) == (size_t)2160 * 101 * 960 * 4);
    CHECK(line_conf_columns_bytes(kLineConfAsBuilt, 2160, 101, 960) > 800u * 1000 * 1000);
    CHECK(line_conf_columns_bytes(kLineConfGate, 4096, 201, 4096) == (size_t)4096 * 201 * 4096 * 4);   // > 2^33
    CHECK(line_conf_columns_bytes(kLineConfGate, 1, 1, 1) == 4);
    CHECK(line_conf_argmax_bytes(kLineConfGate, 3, 5) == 60);
    CHECK(line_conf_argmax_bytes(kLineConfAsBuilt, 65535, 65536) == (size_t)65535 * 65536 * 4);
    CHECK(line_conf_columns_bytes(kLineConfGate, 0, 5, 5) == 0 && line_conf_columns_bytes(kLineConfGate, 5, -1, 5) == 0);
    CHECK(line_conf_argmax_bytes(kLineConfGate, 5, 0) == 0);

    // the #ifdef chain of core.hpp:1097-1103: C_d first, then C_l in the gating mode alone, else the edge mask
    CHECK(sweep_gate(false, kLineConfOff) == kGateEdgeMask);
    CHECK(sweep_gate(false, kLineConfAsBuilt) == kGateEdgeMask);
    CHECK(sweep_gate(false, kLineConfGate) == kGateLineConf);
    for (int mode = 0; mode <= 2; mode++)
        CHECK(sweep_gate(true, mode) == kGateDispConf);

    std::printf("line confidence plan tests ok\n");
    return 0;
}
