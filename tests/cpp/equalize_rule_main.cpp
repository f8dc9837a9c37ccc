// The rule of the per-view equalisation (csrc/k19_equalize_rule.hpp) as a stand-alone host program: g++ compiles the header
// alone, with -ffp-contract=off, and restates whole fields with it.  tests/test_equalize_cpu.py writes the cases and
// compares the output with tests/equalize_ref.py byte for byte.
//
//   equalize_rule_main <cases.bin> <out.bin>
// cases.bin: per case int32 {elem (0 f32, 1 u8, 2 u16), V, S, U, C, mode, ref_view, joint}, float32 {hi, max_gain}, then
//            V * S * U * C float32.
// out.bin:   per case S * C * 3 uint64 (n, s1, s2), S * C * 2 float32 (a, b), V * S * U * C float32 (the applied field).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "k19_equalize_rule.hpp"

using namespace rslf;

int main(int argc, char** argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]);
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) {
        std::fprintf(stderr, "cannot open the files\n");
        return 2;
    }
    int cases = 0;
    int32_t head[8];
    while (std::fread(head, sizeof(int32_t), 8, in) == 8) {
        const int elem = head[0], V = head[1], S = head[2], U = head[3], C = head[4], mode = head[5], ref_view = head[6], joint = head[7];
        float hg[2];
        if (elem < 0 || elem > 2 || V < 1 || S < 1 || U < 1 || (C != 1 && C != 3) || !eq_mode_ok(mode) || ref_view < -1 || ref_view >= S ||
            (joint && C != 3) || std::fread(hg, sizeof(float), 2, in) != 2 || !eq_hi_ok(hg[0]) || !eq_max_gain_ok(hg[1])) {
            std::fprintf(stderr, "case %d: bad header\n", cases);
            return 1;
        }
        std::vector<float> x((size_t)V * S * U * C), y(x.size());
        if (std::fread(x.data(), sizeof(float), x.size(), in) != x.size()) {
            std::fprintf(stderr, "case %d: short input\n", cases);
            return 1;
        }
        const float hi = elem == 0 ? hg[0] : eq_hi_int(elem == 1 ? 1 : 2);
        const float k = eq_quant_scale(hi);
        std::vector<uint64_t> stats((size_t)S * C * kEqStats, 0);
        for (int v = 0; v < V; v++)
            for (int s = 0; s < S; s++)
                for (int u = 0; u < U; u++)
                    for (int c = 0; c < C; c++) {
                        uint64_t* t = &stats[((size_t)s * C + c) * kEqStats];
                        eq_count(x[(((size_t)v * S + s) * U + u) * C + c], hi, k, &t[0], &t[1], &t[2]);
                    }
        std::vector<float> a_b((size_t)S * C * 2);
        eq_coefficients(stats.data(), S, C, hi, mode, ref_view, joint, hg[1], a_b.data());
        for (int v = 0; v < V; v++)
            for (int s = 0; s < S; s++)
                for (int u = 0; u < U; u++)
                    for (int c = 0; c < C; c++) {
                        const size_t i = (((size_t)v * S + s) * U + u) * C + c;
                        const float a = a_b[((size_t)s * C + c) * 2], b = a_b[((size_t)s * C + c) * 2 + 1];
                        y[i] = elem == 0 ? eq_apply<false>(x[i], a, b, hi) : eq_apply<true>(x[i], a, b, hi);
                        // what the rule promises by itself: a NaN stays, everything else ends inside [0, hi] unless copied
                        const bool nan_kept = x[i] != x[i] && y[i] != y[i];
                        const bool copied = a == 1.0f && b == 0.0f && y[i] == x[i];
                        if (!nan_kept && !copied && !(y[i] >= 0.0f && y[i] <= hi)) {
                            std::fprintf(stderr, "case %d: sample %zu breaks the rule's own promises\n", cases, i);
                            return 1;
                        }
                    }
        // the reference view is exactly (1, 0); the clamp holds
        const float gmax = hg[1];
        for (int s = 0; s < S; s++)
            for (int c = 0; c < C; c++) {
                const float a = a_b[((size_t)s * C + c) * 2], b = a_b[((size_t)s * C + c) * 2 + 1];
                if ((s == ref_view && (a != 1.0f || b != 0.0f)) || !(a >= (float)(1.0 / (double)gmax) && a <= gmax)) {
                    std::fprintf(stderr, "case %d: view %d channel %d: a = %g, b = %g\n", cases, s, c, (double)a, (double)b);
                    return 1;
                }
            }
        if (std::fwrite(stats.data(), sizeof(uint64_t), stats.size(), out) != stats.size() ||
            std::fwrite(a_b.data(), sizeof(float), a_b.size(), out) != a_b.size() || std::fwrite(y.data(), sizeof(float), y.size(), out) != y.size())
            return 1;
        cases++;
    }
    std::fclose(in);
    if (std::fclose(out) != 0)
        return 1;
    std::printf("equalize rule: %d cases ok\n", cases);
    return 0;
}
