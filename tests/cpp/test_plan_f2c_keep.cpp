// The host-side decisions of a kept fine-to-coarse run (rslf_plan.hpp: f2c_validity_by_rule, volume_pitch / volume_bytes,
// f2c_kept_level_bytes / f2c_kept_bytes), compiled with g++ alone and run under AddressSanitizer / UBSan
// (tests/test_f2c_keep_cpu.py).
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

// dc.hpp:893-915, written out once more, branch by branch
static F2cValidity chain(bool accept_all, bool use_disp, int mode)
{
    if (accept_all)
        return kValidAll;          // :911
    if (use_disp)
        return kValidDispConf;     // :902
    if (mode == kLineConfGate)
        return kValidLineConf;     // :904
    return kValidEdgeConf;         // :906
}

int main()
{
    CHECK(kF2cValidCompat == RSLF_F2C_VALID_COMPAT && kF2cValidReference == RSLF_F2C_VALID_REFERENCE);
    CHECK(f2c_validity_rule_ok(0) && f2c_validity_rule_ok(1) && !f2c_validity_rule_ok(-1) && !f2c_validity_rule_ok(2));

    // all 2 x 2 x 3 x 2 combinations of (accept_all, use_disp, line_mode, rule)
    int n = 0, differ = 0;
    for (int accept = 0; accept <= 1; accept++)
        for (int disp = 0; disp <= 1; disp++)
            for (int mode = kLineConfOff; mode <= kLineConfGate; mode++)
                for (int rule = kF2cValidCompat; rule <= kF2cValidReference; rule++) {
                    const F2cValidity got = f2c_validity_by_rule(accept != 0, disp != 0, mode, rule);
                    if (rule == kF2cValidCompat) {
                        CHECK(got == f2c_validity(accept != 0, disp != 0, mode));   // row for row the table of the other entries
                        CHECK(got != kValidDispConf);                               // which never reads C_d
                    } else {
                        CHECK(got == chain(accept != 0, disp != 0, mode));
                        differ += got != f2c_validity(accept != 0, disp != 0, mode);
                    }
                    n++;
                }
    CHECK(n == 24);
    CHECK(differ == 3);   // the two rules differ under use_disp_confidence_score without accept_all, in every line mode, and nowhere else
    CHECK(f2c_validity_by_rule(false, true, kLineConfGate, kF2cValidReference) == kValidDispConf);   // C_d comes before C_l
    CHECK(f2c_validity_by_rule(false, true, kLineConfGate, kF2cValidCompat) == kValidEdgeConf);
    CHECK(f2c_validity_by_rule(true, true, kLineConfOff, kF2cValidReference) == kValidAll);

    // a volume's slab: rows of `pitch` pixels, a multiple of 64 and > U
    CHECK(volume_pitch(1) == 64 && volume_pitch(63) == 64 && volume_pitch(64) == 128 && volume_pitch(130) == 192);
    CHECK(volume_bytes(44, 5, 64, 1) == (size_t)44 * 5 * 128 * 4);
    CHECK(volume_bytes(44, 5, 64, 3) == (size_t)44 * 5 * 128 * 3 * 4);
    CHECK(volume_bytes(0, 5, 64, 1) == 0 && volume_bytes(44, 5, 64, 0) == 0);
    CHECK(volume_bytes(2160, 201, 3840, 3) == (size_t)2160 * 201 * 3 * 3904 * 4);   // > 2^34: size_t throughout
    CHECK(volume_bytes(2160, 201, 3840, 3) > ((size_t)1 << 34));

    // a kept level: depth, C_e, C_d as floats, validity as bytes, C_l with a line mode, the volume when kept
    const LevelDims d0{44, 64};
    const size_t n0 = (size_t)5 * 44 * 64;
    CHECK(f2c_kept_level_bytes(5, 1, d0, kLineConfOff, false) == n0 * 13);
    CHECK(f2c_kept_level_bytes(5, 1, d0, kLineConfAsBuilt, false) == n0 * 17);
    CHECK(f2c_kept_level_bytes(5, 1, d0, kLineConfGate, false) == n0 * 17);
    CHECK(f2c_kept_level_bytes(5, 3, d0, kLineConfOff, true) == n0 * 13 + volume_bytes(44, 5, 64, 3));
    CHECK(f2c_kept_level_bytes(0, 1, d0, kLineConfOff, true) == 0);
    CHECK(f2c_kept_level_bytes(5, 1, LevelDims{0, 64}, kLineConfOff, true) == 0);

    // the whole run: case A's pyramid 44 x 64, 22 x 32, 11 x 16 and the two fused planes
    const std::vector<LevelDims> dims = f2c_pyramid(44, 64, -1);
    CHECK(dims.size() == 3 && dims[1].V == 22 && dims[1].U == 32 && dims[2].V == 11 && dims[2].U == 16);
    const size_t n1 = (size_t)5 * 22 * 32, n2 = (size_t)5 * 11 * 16;
    CHECK(f2c_kept_bytes(5, 1, dims, kLineConfOff, false) == (n0 + n1 + n2) * 13 + n0 * 5);
    CHECK(f2c_kept_bytes(5, 1, dims, kLineConfGate, true) ==
          (n0 + n1 + n2) * 17 + n0 * 5 + volume_bytes(44, 5, 64, 1) + volume_bytes(22, 5, 32, 1) + volume_bytes(11, 5, 16, 1));
    CHECK(f2c_kept_bytes(5, 1, std::vector<LevelDims>(), kLineConfOff, true) == 0);
    // a field a user runs (101 views of 960 x 540, 3 channels): about 2 GB with volumes, 1.2 GB without; 201 views of
    // 3840 x 2160 are past 2^34 -- size_t throughout
    CHECK(f2c_kept_bytes(101, 3, f2c_pyramid(540, 960, -1), kLineConfOff, true) > (size_t)2000 * 1000 * 1000);
    CHECK(f2c_kept_bytes(101, 3, f2c_pyramid(540, 960, -1), kLineConfOff, false) < (size_t)1200 * 1000 * 1000);
    CHECK(f2c_kept_bytes(201, 3, f2c_pyramid(2160, 3840, -1), kLineConfOff, false) > ((size_t)1 << 34));

    std::printf("kept fine-to-coarse plan tests ok\n");
    return 0;
}
