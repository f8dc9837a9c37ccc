// The rule of the derivative channels (csrc/k17_derivative_rule.hpp) as a stand-alone host program: g++ compiles the header
// alone, with -ffp-contract=off, and restates whole fields with it.  tests/test_derivative_cpu.py writes the cases and
// compares the output with tests/derivative_ref.py bit for bit.
//
//   derivative_rule_main <cases.bin> <out.bin>
// cases.bin: per case int32 {elem (0 f32, 1 u8, 2 u16), V, S, U}, float32 {weight, hi}, then V * S * U float32.
// out.bin:   per case V * S * U * 3 float32: (x, fu, fv) per pixel.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "k17_derivative_rule.hpp"

using namespace rslf;

template <bool INTEGER>
static void restate(const std::vector<float>& x, int V, int S, int U, float h, float hi, std::vector<float>& out)
{
    const auto at = [&](int v, int s, int u) { return x[((size_t)v * S + s) * U + u]; };
    for (int v = 0; v < V; v++)
        for (int s = 0; s < S; s++)
            for (int u = 0; u < U; u++) {
                float* o = &out[(((size_t)v * S + s) * U + u) * kDerivativeChannels];
                o[0] = at(v, s, u);
                o[1] = derivative_feature<INTEGER>(at(v, s, derivative_right(u, U)), at(v, s, derivative_left(u)), h, hi);
                o[2] = derivative_feature<INTEGER>(at(derivative_right(v, V), s, u), at(derivative_left(v), s, u), h, hi);
            }
}

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
    int32_t head[4];
    while (std::fread(head, sizeof(int32_t), 4, in) == 4) {
        const int elem = head[0], V = head[1], S = head[2], U = head[3];
        float wh[2];
        if (elem < 0 || elem > 2 || V < 1 || S < 1 || U < 1 || std::fread(wh, sizeof(float), 2, in) != 2) {
            std::fprintf(stderr, "case %d: bad header\n", cases);
            return 1;
        }
        std::vector<float> x((size_t)V * S * U), y(x.size() * kDerivativeChannels);
        if (std::fread(x.data(), sizeof(float), x.size(), in) != x.size()) {
            std::fprintf(stderr, "case %d: short input\n", cases);
            return 1;
        }
        const float h = derivative_half_weight(wh[0]);
        const float hi = elem == 0 ? wh[1] : derivative_hi_int(elem == 1 ? 1 : 2);
        if (elem == 0)
            restate<false>(x, V, S, U, h, hi, y);
        else
            restate<true>(x, V, S, U, h, hi, y);
        // what the rule promises by itself: channel 0 is the source, the features are >= 0 and <= hi, and a row or a
        // field of one pixel has no derivative
        for (size_t i = 0; i < x.size(); i++) {
            const float* o = &y[i * kDerivativeChannels];
            const bool same = o[0] == x[i] || (o[0] != o[0] && x[i] != x[i]);
            if (!same || !(o[1] >= 0.0f && o[1] <= hi) || !(o[2] >= 0.0f && o[2] <= hi) || (U == 1 && o[1] != 0.0f) ||
                (V == 1 && o[2] != 0.0f)) {
                std::fprintf(stderr, "case %d: pixel %zu breaks the rule's own promises\n", cases, i);
                return 1;
            }
        }
        if (std::fwrite(y.data(), sizeof(float), y.size(), out) != y.size())
            return 1;
        cases++;
    }
    std::fclose(in);
    if (std::fclose(out) != 0)
        return 1;
    std::printf("derivative rule: %d cases ok\n", cases);
    return 0;
}
