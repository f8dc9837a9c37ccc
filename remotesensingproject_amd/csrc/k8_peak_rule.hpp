// The peaks of one pixel's score row, stated once for the device (k8_peaks.hpp, k8_score_peaks) and for the host
// (tests/cpp/test_plan_peaks.cpp).  No HIP include: g++ compiles it alone.
//
// A row s[0..D-1] is offered in ascending d.  j is a CANDIDATE iff (j == 0 || s[j] > s[j-1]) && (j == D-1 || s[j] >= s[j+1]):
// the first element of each local maximum or plateau.  The first global maximum is always one and its two neighbours never
// are, so no distance rule is needed.  The WINNER i1 is the candidate with the largest score, the first one on ties -- the
// scan's arg max; the RUNNER-UP i2 the largest among the others, the first one on ties (a later candidate as high as the
// winner is a legitimate runner-up); with no other candidate i2 = -1 and its score 0.  The SUB-GRID offset is the vertex of
// the parabola through the winner and its two neighbours, in grid steps, clamped to half a step; 0 at the ends of the grid
// and where the three points lie on a line.
//
// One pass, a window of three values, nothing indexed by a result: a row of NaNs ends with i1 = -1 and touches no memory.
//
// Arithmetic contract: every float operation is one IEEE binary32 operation in the order written.  Host code
// that includes this header is built with -ffp-contract=off.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RSLF_PEAK_FN __host__ __device__ __forceinline__
#else
#define RSLF_PEAK_FN inline
#endif

namespace rslf {

struct PeakResult {
    int32_t idx;          // i1, -1: the row had no candidate (NaNs)
    float score;          // s[i1]
    float disp;           // the grid value of i1 moved by the sub-grid offset
    int32_t runner_idx;   // i2, -1: no other candidate
    float runner_score;   // s[i2], 0 without one
};

// The sub-grid disparity of a winner i1 whose score is s1 and whose neighbours scored a (i1 - 1) and c (i1 + 1): the grid value
// moved by the vertex of the parabola through the three points.  Stated once: PeakScan::finish below has the three scores
// from a whole row, k9_subgrid_refine (k9_subgrid.hpp) from re-scoring the two neighbours.  a and c are not read at the ends
// of the grid.  lo, hi: the pixel's disparity range; the grid value is the scan's hypothesis() (k2_scan.hpp).
RSLF_PEAK_FN float peak_disp(int i1, int D, float lo, float hi, float a, float s1, float c)
{
    const float range = hi - lo, denom = (float)(D - 1);
    const float num_d = (float)i1 * range;
    const float quo = num_d / denom;
    const float Dd = lo + quo;
    float delta = 0.0f;
    if (i1 > 0 && i1 < D - 1) {
        const float num = a - c;
        const float t = a + c;
        const float bb = s1 + s1;
        const float den = t - bb;
        const float den2 = den + den;
        delta = den2 == 0.0f ? 0.0f : num / den2;
        delta = fminf(fmaxf(delta, -0.5f), 0.5f);
    }
    const float step = range / denom;
    const float move = delta * step;
    return Dd + move;
}

struct PeakScan {
    float before, last;   // s[d-2], s[d-1] once s[d-1] has been offered
    int i1, i2;
    float s1, s2;
    float a, c;           // s[i1-1], s[i1+1] (unset at the ends of the grid, where nothing reads them)

    RSLF_PEAK_FN void init()
    {
        before = last = 0.0f;
        i1 = i2 = -1;
        s1 = s2 = a = c = 0.0f;
    }
    // j, whose score is `last`, is judged once its right neighbour is known (or there is none).  Selects, not branches:
    // on the device every lane of a wave walks a row of its own.
    RSLF_PEAK_FN void judge(int j, float next, bool has_next)
    {
        // (| and & on the tests and values, not references, in the selects: nothing here is control flow or an address)
        const float b0 = before, b1 = last, o_s1 = s1, o_s2 = s2, o_a = a, o_c = c;
        const int o_i1 = i1, o_i2 = i2;
        const bool candidate = ((j == 0) | (b1 > b0)) & ((!has_next) | (b1 >= next));
        // a new winner: the old one is then the best of the others (s1 >= s2, and it came first)
        const bool wins = candidate & ((o_i1 < 0) | (b1 > o_s1));
        const bool second = candidate & !wins & ((o_i2 < 0) | (b1 > o_s2));
        const int i2_else = second ? +j : +o_i2;
        const float s2_else = second ? +b1 : +o_s2;
        i2 = wins ? +o_i1 : +i2_else;
        s2 = wins ? +o_s1 : +s2_else;
        i1 = wins ? +j : +o_i1;
        s1 = wins ? +b1 : +o_s1;
        a = wins ? +b0 : +o_a;
        c = wins ? +next : +o_c;
    }
    // s = s[d]; d ascends from 0, one call each
    RSLF_PEAK_FN void offer(float s, int d)
    {
        if (d > 0)
            judge(d - 1, s, true);
        before = last;
        last = s;
    }
    // After all D >= 1 values.  lo, hi: the pixel's disparity range (peak_disp).
    RSLF_PEAK_FN PeakResult finish(int D, float lo, float hi)
    {
        judge(D - 1, 0.0f, false);
        PeakResult r;
        r.idx = i1, r.score = s1;
        r.runner_idx = i2, r.runner_score = i2 < 0 ? 0.0f : s2;
        r.disp = peak_disp(i1, D, lo, hi, a, s1, c);
        return r;
    }
};

// A whole row at once (the host's form; the kernel offers block by block)
RSLF_PEAK_FN PeakResult peak_row(const float* s, int D, float lo, float hi)
{
    PeakScan scan;
    scan.init();
    for (int d = 0; d < D; d++)
        scan.offer(s[d], d);
    return scan.finish(D, lo, hi);
}

}  // namespace rslf
