// The two pieces of the peak rule (k8_peak_rule.hpp) that a row spread over the lanes of a wave needs and that are not
// shuffles: the candidate test of one element given its two neighbours, and the merge of two (winner, runner-up) pairs.
// Stated once for the device (k10_sweep_peaks.hpp, k10_peaks_list) and for the host (tests/cpp/test_plan_sweep_peaks.cpp,
// which folds rows in chunks and requires peak_row's results).  No HIP include: g++ compiles it alone.
//
// The rule as an order: among the candidates of a row, a comes BEFORE b iff s[a] > s[b], or s[a] == s[b] and a < b.  The
// winner is the first candidate in that order and the runner-up the second -- which is what PeakScan's one pass in ascending
// d computes (a later candidate wins on a larger score only; a displaced winner is the best of the others).  The first two
// elements of a totally ordered set can be found from the first two of any two parts of it: top2_merge is associative and
// commutative, so the row may be cut anywhere and the parts merged in any order.  A NaN is never a candidate (both tests
// are false on it, and no row has j == 0 == D - 1: D >= 2), so the order is total on what it is asked about.
#pragma once

#include "k8_peak_rule.hpp"

namespace rslf {

struct Top2 {
    int32_t i1;   // the part's best candidate, -1: it has none (then i2 == -1 too)
    float s1;
    int32_t i2;   // its second best, -1: none
    float s2;
};

RSLF_PEAK_FN Top2 top2_none()
{
    Top2 t;
    t.i1 = t.i2 = -1;
    t.s1 = t.s2 = 0.0f;
    return t;
}

// j of a row of D, whose score is cur and whose neighbours scored prev (j - 1) and next (j + 1); prev is not read at j == 0,
// next not at j == D - 1.  (| and & on the tests: selects, as PeakScan::judge.)
RSLF_PEAK_FN bool is_candidate(float prev, float cur, float next, int j, int D)
{
    return ((j == 0) | (cur > prev)) & ((j == D - 1) | (cur >= next));
}

// The part that holds element j alone
RSLF_PEAK_FN Top2 top2_one(bool candidate, int j, float s)
{
    Top2 t = top2_none();
    t.i1 = candidate ? j : -1;
    t.s1 = candidate ? s : 0.0f;
    return t;
}

// (ia, sa) comes before (ib, sb) in the rule's order; "none" (-1) comes after everything
RSLF_PEAK_FN bool top2_before(int ia, float sa, int ib, float sb)
{
    return (ia >= 0) & ((ib < 0) | (sa > sb) | ((sa == sb) & (ia < ib)));
}

RSLF_PEAK_FN Top2 top2_merge(const Top2 a, const Top2 b)
{
    // the winner's side keeps its runner-up in play; the other side's winner is the only one of that side that can be second
    const bool a_first = top2_before(a.i1, a.s1, b.i1, b.s1);
    const int wi = a_first ? +a.i1 : +b.i1, li = a_first ? +b.i1 : +a.i1, ri = a_first ? +a.i2 : +b.i2;
    const float ws = a_first ? +a.s1 : +b.s1, ls = a_first ? +b.s1 : +a.s1, rs = a_first ? +a.s2 : +b.s2;
    const bool l_second = top2_before(li, ls, ri, rs);
    Top2 t;
    t.i1 = wi, t.s1 = ws;
    t.i2 = l_second ? +li : +ri;
    t.s2 = l_second ? +ls : +rs;
    return t;
}

// What rslf_peaks reports of a whole row's pair: no runner-up scores 0
RSLF_PEAK_FN float top2_runner_score(const Top2 t) { return t.i2 < 0 ? 0.0f : t.s2; }

}  // namespace rslf
