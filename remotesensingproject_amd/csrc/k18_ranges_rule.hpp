// K18, the rule: a level's per-pixel hypothesis ranges [dmin, dmax] in the frame dilated along u by f.  Host + device, no
// HIP in it: g++ compiles it alone (tests/cpp/ranges_rule_main.cpp), the kernel (k18_level_dilate.hpp) and the host loop
// (rslf_planes_dilate_ranges_u_host) run the same functions.
//
// Column j = i * f + p of the dilated row lies between the source columns i and i + 1 (p > 0) or on column i (p == 0).  On
// a source column the range is the column's, bit for bit.  Between two it is their union, min of the lower bounds and max
// of the upper ones, so no hypothesis either neighbour allowed is lost.  min and max are fminf / fmaxf with what C leaves
// open stated: of two equal values (-0.0f and +0.0f compare equal) the LEFT neighbour's bits, and a NaN loses to a number.
#pragma once

#if defined(__HIPCC__)
#define RSLF_K18_HD __host__ __device__
#else
#define RSLF_K18_HD
#endif

namespace rslf {

RSLF_K18_HD inline float ranges_min(float a, float b) { return (a <= b || b != b) ? a : b; }
RSLF_K18_HD inline float ranges_max(float a, float b) { return (a >= b || b != b) ? a : b; }

// The source column i and phase p of the dilated column j (0 <= j <= f * (U - 1)); p > 0 implies i + 1 <= U - 1.
RSLF_K18_HD inline void ranges_source(int j, int f, int* i, int* p)
{
    *i = j / f;
    *p = j - *i * f;
}

// Column j of the dilated lower / upper bound row from the source row of U columns.
RSLF_K18_HD inline float ranges_lower(const float* dmin, int j, int f)
{
    int i, p;
    ranges_source(j, f, &i, &p);
    return p == 0 ? dmin[i] : ranges_min(dmin[i], dmin[i + 1]);
}
RSLF_K18_HD inline float ranges_upper(const float* dmax, int j, int f)
{
    int i, p;
    ranges_source(j, f, &i, &p);
    return p == 0 ? dmax[i] : ranges_max(dmax[i], dmax[i + 1]);
}

// The span of a row of `width` columns that store group g covers when the row starts `a` floats (0..3) past a 16-byte
// boundary: the columns [4 g - a, 4 g - a + 4) cut to the row.  A whole span (count == 4) starts on a 16-byte boundary and
// goes out as one 16-byte store; the cut ones at a row's two ends go out one float at a time.  a = 0 for every row when the
// rows are taken as unaligned (then every span goes out one float at a time).
struct RangesSpan {
    int first, count;
};
RSLF_K18_HD inline RangesSpan ranges_span(long long g, int a, int width)
{
    long long lo = 4 * g - a, hi = lo + 4;
    if (lo < 0)
        lo = 0;
    if (hi > width)
        hi = width;
    RangesSpan s;
    s.first = (int)lo;
    s.count = hi > lo ? (int)(hi - lo) : 0;
    return s;
}
RSLF_K18_HD inline long long ranges_groups(int a, int width) { return ((long long)width + a + 3) / 4; }

}  // namespace rslf
