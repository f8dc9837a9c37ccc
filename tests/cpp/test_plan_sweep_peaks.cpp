// The host-side pieces of the 2-D sweep's peaks mode, compiled with g++ alone and run under AddressSanitizer / UBSan
// (tests/test_sweep_peaks_cpu.py): rslf_plan_sweep_peaks.hpp -- which form of the step a visit queues, the list form's
// fixed grid, the sizes of the step's own buffers -- and k10_peak_merge.hpp, the two pieces of the cross-lane peak rule that
// are not shuffles.  Rows are folded the way k10_peaks_list folds them -- chunks of W elements, the last element of a chunk
// judged once the next chunk's first is known, the chunks' pairs merged -- for W = 64 and other widths, in several merge
// orders, and must give peak_row's idx, score, runner_idx and runner_score (k8_peak_rule.hpp) bit for bit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "k10_peak_merge.hpp"
#include "rslf_plan_sweep_peaks.hpp"

using namespace rslf;
using namespace rslf::plan;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

// The pairs of the chunks [k W, (k + 1) W) of a row, as the kernel's rounds make them: an element is judged in its own chunk
// unless it is the chunk's last and the row goes on; then the next chunk takes it (the carried score and its left neighbour).
static std::vector<Top2> chunk_pairs(const std::vector<float>& s, int W)
{
    const int D = (int)s.size();
    std::vector<Top2> out;
    float c_prev = 0.0f, c_cur = 0.0f;
    for (int d0 = 0; d0 < D; d0 += W) {
        Top2 acc = top2_none();
        if (d0 > 0)   // the element carried from the chunk before
            acc = top2_one(is_candidate(c_prev, c_cur, s[d0], d0 - 1, D), d0 - 1, c_cur);
        for (int lane = 0; lane < W && d0 + lane < D; lane++) {
            const int d = d0 + lane;
            const float prev = lane == 0 ? c_cur : s[d - 1];
            const float next = d + 1 < D && lane + 1 < W ? s[d + 1] : -12345.0f;   // (not read where it is not known)
            const bool now = lane != W - 1 || d == D - 1;
            acc = top2_merge(acc, top2_one(now && is_candidate(prev, s[d], next, d, D), d, s[d]));
        }
        const int last = d0 + W - 1;
        if (last < D) {
            c_prev = W == 1 ? c_cur : s[last - 1];
            c_cur = s[last];
        }
        out.push_back(acc);
    }
    return out;
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }

static void expect(const Top2& t, const PeakResult& want, const char* what, int W)
{
    const bool ok = t.i1 == want.idx && same_bits(t.s1, want.score) && t.i2 == want.runner_idx &&
                    same_bits(top2_runner_score(t), want.runner_score);
    if (!ok) {
        std::printf("FAILED %s, width %d: got (%d, %g, %d, %g), peak_row gives (%d, %g, %d, %g)\n", what, W, t.i1, t.s1, t.i2,
                    top2_runner_score(t), want.idx, want.score, want.runner_idx, want.runner_score);
        std::exit(1);
    }
}

static Top2 tree(const std::vector<Top2>& p, size_t a, size_t b)   // [a, b), b > a
{
    if (b - a == 1)
        return p[a];
    const size_t m = a + (b - a) / 2;
    return top2_merge(tree(p, a, m), tree(p, m, b));
}

static const int kWidths[] = {64, 1, 2, 3, 5, 7, 16, 63, 65, 200};

static void check_row(const std::vector<float>& s, const char* what)
{
    const int D = (int)s.size();
    const PeakResult want = peak_row(s.data(), D, 0.0f, 1.0f);
    for (int W : kWidths) {
        const std::vector<Top2> p = chunk_pairs(s, W);
        Top2 left = top2_none(), right = top2_none();
        for (size_t i = 0; i < p.size(); i++)
            left = top2_merge(left, p[i]);
        for (size_t i = p.size(); i-- > 0;)
            right = top2_merge(p[i], right);
        Top2 swapped = top2_none();   // commuted operands, the butterfly's other lane
        for (size_t i = 0; i < p.size(); i++)
            swapped = top2_merge(p[i], swapped);
        expect(left, want, what, W);
        expect(right, want, what, W);
        expect(swapped, want, what, W);
        expect(tree(p, 0, p.size()), want, what, W);
    }
}

static unsigned lcg(unsigned& x) { return x = x * 1664525u + 1013904223u; }

int main()
{
    // ---- the plan ----------------------------------------------------------------------------------------------------
    const long long small = 6 * 80, c3 = 540ll * 960, limit = 2147483647ll;
    for (int first = 0; first < 2; first++)
        for (int listed = 0; listed < 2; listed++)
            for (int hook = 0; hook < 2; hook++)
                CHECK(sweep_peaks_form(false, first, listed, hook, small) == kPeaksNone);
    CHECK(sweep_peaks_form(true, true, false, 1, small) == kPeaksDense);    // the first visit: nothing is listed yet
    CHECK(sweep_peaks_form(true, true, true, 1, small) == kPeaksDense);     // first wins over a stale `listed`
    CHECK(sweep_peaks_form(true, false, true, 1, small) == kPeaksList);     // a sparse visit
    CHECK(sweep_peaks_form(true, false, true, 1, c3) == kPeaksList);
    CHECK(sweep_peaks_form(true, false, false, 1, small) == kPeaksDense);   // "force_packed" = 0
    CHECK(sweep_peaks_form(true, false, true, 0, small) == kPeaksDense);    // "peaks_list" = 0
    CHECK(sweep_peaks_form(true, false, true, 1, limit) == kPeaksList);
    CHECK(sweep_peaks_form(true, false, true, 1, limit + 1) == kPeaksDense);
    {
        bool first = true, listed = false;
        int dense = 0, list = 0;
        for (int visit = 0; visit < 5; visit++) {
            const PeaksForm f = sweep_peaks_form(true, first, listed, 1, small);
            dense += f == kPeaksDense, list += f == kPeaksList;
            first = false, listed = true;   // what rslf_sweep_visit_finish leaves
        }
        CHECK(dense == 1 && list == 4);
    }
    // the list form's grid: a wave per entry, four waves a workgroup, eight workgroups a compute unit at most
    CHECK(peaks_list_blocks(6, 80, 256) == 120);
    CHECK(peaks_list_blocks(1, 1, 256) == 1 && peaks_list_blocks(1, 4, 256) == 1 && peaks_list_blocks(1, 5, 256) == 2);
    CHECK(peaks_list_blocks(540, 960, 256) == 2048 && peaks_list_blocks(540, 960, 0) == 2048);
    CHECK(peaks_list_blocks(540, 960, 8) == 64);
    CHECK(peaks_list_blocks(46340, 46340, 256) == 2048);   // close to INT32_MAX pixels: no overflow on the way
    CHECK(peaks_list_blocks(0, 80, 256) == 1 && peaks_list_blocks(6, -1, 256) == 1);
    CHECK((long long)peaks_list_blocks(65535, 32768, 65536) * kPeaksListWaves <= (1ll << 22));   // the kernel's unsigned stride
    CHECK(peaks_list_rounds(2) == 1 && peaks_list_rounds(64) == 1 && peaks_list_rounds(65) == 2 && peaks_list_rounds(129) == 3);
    CHECK(peaks_list_rounds(0) == 0);
    // the step's own buffers
    CHECK(sweep_peaks_list_bytes(false, 540, 960) == 0 && sweep_peaks_list_bytes(true, 540, 960) == (size_t)540 * 960 * 4);
    CHECK(sweep_peaks_list_bytes(true, 65535, 65536) == (size_t)65535 * 65536 * 4);
    CHECK(sweep_peaks_mask_bytes(true, 540, 960) == (size_t)540 * 960 && sweep_peaks_mask_bytes(false, 540, 960) == 0);
    CHECK(sweep_peaks_count_offset_total(6) == 24 && sweep_peaks_count_offset_total(7) == 32);   // the total is 8-byte aligned
    CHECK(sweep_peaks_count_bytes(true, 7, 80) == 40 && sweep_peaks_count_bytes(false, 7, 80) == 0);
    CHECK(sweep_peaks_count_bytes(true, 0, 80) == 0 && sweep_peaks_list_bytes(true, 5, 0) == 0);
    // the dense form's passes: whole planes where the budget holds them, at least one scanline, never more than V
    CHECK(sweep_peaks_pass_rows(6, 80, 9, (size_t)256 << 20) == 6);
    CHECK(sweep_peaks_pass_rows(6, 80, 9, 4096) == 1);             // a scanline's rows are 2880 bytes: one fits
    CHECK(sweep_peaks_pass_rows(6, 80, 9, 2 * 2880) == 2);
    CHECK(sweep_peaks_pass_rows(6, 80, 9, 1) == 1);
    CHECK(sweep_peaks_staging_bytes(6, 80, 9, 2 * 2880) == 2 * 2880);
    CHECK(sweep_peaks_staging_bytes(6, 80, 9, (size_t)256 << 20) == (size_t)6 * 2880);
    CHECK(sweep_peaks_staging_bytes(6, 80, 0, 4096) == 0);

    // ---- the candidate test ------------------------------------------------------------------------------------------
    CHECK(is_candidate(-1.0f, 1.0f, 0.0f, 0, 4) && is_candidate(9.0f, 1.0f, 1.0f, 0, 4));   // j == 0: prev is not read
    CHECK(!is_candidate(0.0f, 1.0f, 2.0f, 0, 4));
    CHECK(is_candidate(0.0f, 1.0f, 9.0f, 3, 4) && !is_candidate(1.0f, 1.0f, 0.0f, 3, 4));   // j == D - 1: next is not read
    CHECK(is_candidate(0.0f, 1.0f, 1.0f, 1, 4) && !is_candidate(1.0f, 1.0f, 1.0f, 1, 4));   // the first of a plateau only

    // ---- the merge ---------------------------------------------------------------------------------------------------
    {
        const Top2 none = top2_none();
        const Top2 a = top2_one(true, 3, 5.0f), b = top2_one(true, 7, 5.0f), c = top2_one(false, 9, 99.0f);
        CHECK(c.i1 == -1 && c.i2 == -1);
        Top2 m = top2_merge(a, b);
        CHECK(m.i1 == 3 && m.i2 == 7 && m.s2 == 5.0f);   // a tie: the smaller d wins, the other is a legitimate runner-up
        m = top2_merge(b, a);
        CHECK(m.i1 == 3 && m.i2 == 7);
        m = top2_merge(none, a);
        CHECK(m.i1 == 3 && m.i2 == -1 && top2_runner_score(m) == 0.0f);
        m = top2_merge(top2_merge(a, none), c);
        CHECK(m.i1 == 3 && m.i2 == -1);
        m = top2_merge(none, none);
        CHECK(m.i1 == -1 && m.i2 == -1);
    }

    // ---- hand-worked rows (tests/peaks_ref.py, HAND) -----------------------------------------------------------------
    {
        struct Hand { const char* name; std::vector<float> s; int i1; float s1; int i2; float s2; };
        const Hand hand[] = {
            {"winner_first", {4, 3, 2, 1}, 0, 4.0f, -1, 0.0f},
            {"winner_last", {1, 2, 3, 4}, 3, 4.0f, -1, 0.0f},
            {"interior", {0, 1, 4, 3, 2}, 2, 4.0f, -1, 0.0f},
            {"runner", {2, 5, 4, 0, 3, 1}, 1, 5.0f, 4, 3.0f},
            {"all_equal", {2, 2, 2, 2}, 0, 2.0f, -1, 0.0f},
            {"two_equal", {1, 1}, 0, 1.0f, -1, 0.0f},
            {"two_rising", {1, 2}, 1, 2.0f, -1, 0.0f},
            {"tied_runner", {1, 5, 1, 5, 0}, 1, 5.0f, 3, 5.0f},
            {"plateaus", {1, 3, 3, 3, 1, 2, 2, 0}, 1, 3.0f, 5, 2.0f},
            {"flat_range", {9, 0, 2, 0, 6, 0, 4}, 0, 9.0f, 4, 6.0f},
            {"late_winner", {0, 3, 0, 2, 4, 7, 6}, 5, 7.0f, 1, 3.0f},
        };
        for (const Hand& h : hand) {
            const PeakResult r = peak_row(h.s.data(), (int)h.s.size(), 0.0f, 1.0f);
            CHECK(r.idx == h.i1 && r.score == h.s1 && r.runner_idx == h.i2 && r.runner_score == h.s2);   // the table is peak_row's
            check_row(h.s, h.name);
        }
    }

    // ---- plateaus across a chunk edge, a runner-up as high as the winner in a later chunk, constant rows -------------
    for (int D : {2, 3, 63, 64, 65, 128, 129}) {
        std::vector<float> s((size_t)D, 0.5f);
        check_row(s, "constant");
        CHECK(peak_row(s.data(), D, 0.0f, 1.0f).runner_idx == -1);
        for (int edge : {63, 64, 65, 127, 128}) {   // a plateau of three that straddles element `edge`
            if (edge + 1 >= D || edge < 1)
                continue;
            std::vector<float> p((size_t)D, 0.0f);
            p[(size_t)edge - 1] = p[(size_t)edge] = p[(size_t)edge + 1] = 2.0f;
            p[0] = 1.0f;
            check_row(p, "plateau across an edge");
            const PeakResult r = peak_row(p.data(), D, 0.0f, 1.0f);
            CHECK(r.idx == edge - 1 && r.runner_idx == 0);
        }
        if (D >= 65) {   // the winner in the first chunk, a candidate as high in a later one
            std::vector<float> t((size_t)D, 0.0f);
            t[5] = 3.0f, t[(size_t)D - 1] = 3.0f, t[40] = 2.0f;
            check_row(t, "tied runner in a later chunk");
            const PeakResult r = peak_row(t.data(), D, 0.0f, 1.0f);
            CHECK(r.idx == 5 && r.runner_idx == D - 1 && r.runner_score == 3.0f);
            t[5] = 0.0f, t[64] = 3.0f;   // ... and the winner on a chunk's first element
            check_row(t, "winner on a chunk's first element");
        }
        // winners forced to both ends
        std::vector<float> up((size_t)D), down((size_t)D);
        for (int d = 0; d < D; d++)
            up[(size_t)d] = (float)d, down[(size_t)d] = (float)(D - d);
        check_row(up, "rising");
        check_row(down, "falling");
    }

    // ---- random rows with planted ties -------------------------------------------------------------------------------
    {
        unsigned seed = 12345u;
        for (int D : {2, 3, 63, 64, 65, 128, 129})
            for (int rep = 0; rep < 60; rep++) {
                std::vector<float> s((size_t)D);
                const unsigned levels = rep % 3 == 0 ? 3u : rep % 3 == 1 ? 17u : 1000u;   // few levels: ties and plateaus everywhere
                for (int d = 0; d < D; d++)
                    s[(size_t)d] = (float)(lcg(seed) >> 8) / 16777216.0f * (float)levels;
                if (levels != 1000u)
                    for (int d = 0; d < D; d++)
                        s[(size_t)d] = (float)(int)s[(size_t)d] * 0.125f;
                // plant the maximum twice, wherever the draw puts it
                const size_t a = lcg(seed) % (unsigned)D, b = lcg(seed) % (unsigned)D;
                s[a] = s[b] = (float)levels + 1.0f;
                check_row(s, "random");
            }
    }

    std::printf("sweep peaks plan tests ok\n");
    return 0;
}
