// The lerp taps of one view offset for a whole tile of pixels on one scanline, stated once for the register scan
// (k2_reg.hpp, scan_reg_body) and for the host (tests/cpp/test_taps.cpp).  No HIP include: g++ compiles it alone.
//
// A sample of pixel u at view offset `off` sits at x = fl(off + u) (core.hpp:552); its taps are floor(x) and floor(x) + 1,
// its weight t = x - floor(x) (interp.hpp:179-181).  For the integer pixels u_first <= u <= u_last of one tile, t and
// floor(x) - u are THE SAME for every u whenever
//   (a) fl(off + u_first) and fl(off + u_last) lie in one binade: its quantum q <= 1/2 divides every u an even number of
//       times, so fl(off + u) = u + round_q(off) and a tie is settled by `off` alone; or
//   (b) fl(fl(off + u_last) - u_last) == off: the sum is exact at the widest pixel, hence at every one.
// Then one entry {address of the first pixel's left tap, t, 1 - t} serves the tile: pixel u reads at the entry's address
// plus (u - u_first) pixels.  `fast` also asks that every sample lies inside the row, 0 < x_first and x_last <= U - 1, so a
// fast sample is never the out-of-range sentinel.
//
// Arithmetic contract: every float operation is the single IEEE binary32 operation scan_reg_body performs.  Host code
// that includes this header is built with -ffp-contract=off.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define RSLF_TAPS_FN __host__ __device__ __forceinline__
#else
#define RSLF_TAPS_FN inline
#endif

namespace rslf {

struct TapEntry {
    int byteoff;    // of the first pixel's left tap, from the EPI's base: (floor(x_first) * C + row) * 4
    float t, omt;   // weight of the right tap and 1 - t, the left tap's (interp.hpp:184)
    bool fast;      // the entry holds for every pixel of the tile
};

RSLF_TAPS_FN uint32_t tap_float_bits(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(x);
#else
    uint32_t b;
    memcpy(&b, &x, sizeof(b));
    return b;
#endif
}

// x - floor(x) and (int)floor(x) for x > 0: v_fract_f32 / v_cvt_flr_i32_f32 on the device (rslf_device.hpp, lerp_weight:
// the subtraction is exact there, so both sides give the same bits)
RSLF_TAPS_FN float tap_fract(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fractf(x);
#else
    return x - floorf(x);
#endif
}
RSLF_TAPS_FN int tap_floor(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int i;
    asm("v_cvt_flr_i32_f32_e32 %0, %1" : "=v"(i) : "v"(x));
    return i;
#else
    return (int)floorf(x);
#endif
}

// `off`: the view offset fl(fl(float(s_hat - s) * D[d]) * slope); [u_first, u_last]: the tile's pixels; U: the row's width;
// C: channels; row_floats: s * stride_s, the view's row within the EPI (32-bit, as the kernel's addresses are).
RSLF_TAPS_FN TapEntry tap_entry(float off, int u_first, int u_last, int U, int C, int row_floats)
{
    const float uf = (float)u_first, ul = (float)u_last;
    const float x_first = off + uf;            // core.hpp:552
    const float x_last = off + ul;
    TapEntry e;
    e.t = tap_fract(x_first);                  // interp.hpp:181
    const int i0 = tap_floor(x_first);         // interp.hpp:179
    e.omt = 1.0f - e.t;
    e.byteoff = (int)((unsigned)(i0 * C + row_floats) << 2);
    const bool inside = x_first > 0.0f && x_last <= (float)(U - 1);
    // (a) one binade: same sign (positive) and same exponent field
    const bool binade = ((tap_float_bits(x_first) ^ tap_float_bits(x_last)) >> 23) == 0;
    // (b) exact at the widest pixel
    const float back = x_last - ul;
    const bool exact = back == off;
    e.fast = inside && (binade || exact);
    return e;
}

// The same entry for a whole ROW: every pixel 0 <= u <= U - 1 whose sample lies inside the row, on every scanline.  Rule (b)
// asked at the row's widest pixel does not depend on the tile: when x_last = fl(off + (U - 1)) is the exact sum, `off` is a
// multiple of x_last's quantum (U - 1 is an integer, the quantum at most 1), so off + u is a multiple of it no larger than
// x_last for every sample inside [0, x_last]: representable, the sum exact.  Then floor(x) - u = floor(off) and
// t = off - floor(off) in every pixel, and {tap offset, t, 1 - t} is a function of the view offset alone.
// The entry is made from x_last, a position inside the row like the ones the lanes compute (positive: fract and the
// floor-convert are used where scan_reg_body uses them), not from `off`, which may be negative.  `exact` also asks
// 1 <= x_last < 2^23 (a row some sample can be inside of; quantum below 1) and that `byteoff` did not wrap.
struct RowExactEntry {
    int byteoff;    // of pixel 0's left tap, from the EPI's base: ((floor(off)) * C + row) * 4 -- negative where floor(off) < 0;
                    // pixel u reads at byteoff + u * C * 4
    float t, omt;
    bool exact;     // the entry holds for every pixel of the row whose sample lies inside it
};

RSLF_TAPS_FN RowExactEntry row_exact_entry(float off, int U, int C, int row_floats)
{
    const float ul = (float)(U - 1);
    const float x_last = off + ul;             // core.hpp:552 at the widest pixel
    const float back = x_last - ul;
    RowExactEntry e;
    const bool sane = x_last >= 1.0f && x_last < 8388608.0f;
    const float xs = sane ? x_last : 1.0f;     // (keeps the conversions below defined)
    e.t = tap_fract(xs);                       // interp.hpp:181
    const int i_last = tap_floor(xs);          // interp.hpp:179
    e.omt = 1.0f - e.t;
    const long long floats = (long long)(i_last - (U - 1)) * C + row_floats;
    e.byteoff = (int)((unsigned)floats << 2);
    const bool fits = floats >= -(1LL << 28) && floats < (1LL << 28);
    e.exact = sane && fits && back == off;     // rule (b) at u = U - 1
    return e;
}

}  // namespace rslf
