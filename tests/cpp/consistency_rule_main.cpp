// The rule header of the cross-view consistency check (csrc/k12_consistency_rule.hpp) as a stand-alone program, for
// tests/test_consistency_cpu.py: planes in from a file, the six result planes out to another, compared there bit for bit
// with the numpy yardstick.  Built by g++ with -ffp-contract=off; no HIP.
//
//   consistency_rule_main IN OUT S V U slope tol radius min_agree has_valid
//   IN:  depth [S][V][U] float32, then (has_valid) valid [S][V][U] uint8
//   OUT: seen, agree, above, below [S][V][U] int32, fused float32, valid uint8
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "k12_consistency_rule.hpp"

int main(int argc, char** argv)
{
    if (argc != 11) {
        fprintf(stderr, "usage: %s IN OUT S V U slope tol radius min_agree has_valid\n", argv[0]);
        return 2;
    }
    const int S = atoi(argv[3]), V = atoi(argv[4]), U = atoi(argv[5]);
    const float slope = strtof(argv[6], nullptr), tol = strtof(argv[7], nullptr);
    const int radius = atoi(argv[8]), min_agree = atoi(argv[9]), has_valid = atoi(argv[10]);
    const size_t n = (size_t)S * V * U;
    std::vector<float> depth(n);
    std::vector<uint8_t> valid(n);
    FILE* in = fopen(argv[1], "rb");
    if (!in || fread(depth.data(), sizeof(float), n, in) != n || (has_valid && fread(valid.data(), 1, n, in) != n)) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    fclose(in);
    std::vector<int32_t> seen(n), agree(n), above(n), below(n);
    std::vector<float> fused(n);
    std::vector<uint8_t> valid_out(n);
    for (int s = 0; s < S; s++)
        for (int v = 0; v < V; v++)
            for (int u = 0; u < U; u++) {
                const rslf::ConsistencyResult r =
                    rslf::consistency_pixel(depth.data(), has_valid ? valid.data() : nullptr, S, V, U, s, v, u, slope, tol, radius, min_agree);
                const size_t o = ((size_t)s * V + v) * U + u;
                seen[o] = r.seen, agree[o] = r.agree, above[o] = r.above, below[o] = r.below;
                fused[o] = r.fused, valid_out[o] = r.valid;
            }
    FILE* out = fopen(argv[2], "wb");
    if (!out)
        return 2;
    bool ok = fwrite(seen.data(), 4, n, out) == n && fwrite(agree.data(), 4, n, out) == n && fwrite(above.data(), 4, n, out) == n &&
              fwrite(below.data(), 4, n, out) == n && fwrite(fused.data(), 4, n, out) == n && fwrite(valid_out.data(), 1, n, out) == n;
    ok = fclose(out) == 0 && ok;
    return ok ? 0 : 2;
}
