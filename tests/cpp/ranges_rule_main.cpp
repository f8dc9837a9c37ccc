// csrc/k18_ranges_rule.hpp compiled alone by g++: the union rule of the level dilation's ranges on cases read from a file.
// Usage: ranges_rule_main cases.bin out.bin.  cases.bin: records of int32 (f, U, rows), then rows * U floats of dmin and
// rows * U of dmax.  out.bin: per case rows * U' floats of the dilated dmin, then of the dilated dmax.  The program itself
// checks phase 0 (the source's bits) and that every read stays inside its row; tests/test_f2c_dilate_cpu.py compares the
// output with numpy bit for bit.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "k18_ranges_rule.hpp"

using namespace rslf;

static uint32_t bits(float x)
{
    uint32_t b;
    memcpy(&b, &x, 4);
    return b;
}

int main(int argc, char** argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "cannot open the files\n");
        return 2;
    }
    int head[3], cases = 0;
    while (fread(head, sizeof(int), 3, in) == 3) {
        const int f = head[0], U = head[1], rows = head[2];
        if (f < 1 || f > 8 || U < 1 || rows < 1) {
            fprintf(stderr, "bad case f=%d U=%d rows=%d\n", f, U, rows);
            return 1;
        }
        // exactly U floats per row, each row its own allocation: a read beyond a row is the sanitizer's to report
        std::vector<std::vector<float>> lo((size_t)rows, std::vector<float>((size_t)U)), hi = lo;
        for (auto* planes : {&lo, &hi})
            for (auto& row : *planes)
                if (fread(row.data(), sizeof(float), (size_t)U, in) != (size_t)U) {
                    fprintf(stderr, "short case\n");
                    return 1;
                }
        const int Ud = f * (U - 1) + 1;
        std::vector<float> olo((size_t)rows * Ud), ohi((size_t)rows * Ud);
        for (int r = 0; r < rows; r++)
            for (int j = 0; j < Ud; j++) {
                int i, p;
                ranges_source(j, f, &i, &p);
                if (i < 0 || i >= U || (p > 0 && i + 1 >= U) || p < 0 || p >= f) {
                    fprintf(stderr, "f=%d U=%d: column %d reads outside its row (i=%d p=%d)\n", f, U, j, i, p);
                    return 1;
                }
                const float a = ranges_lower(lo[(size_t)r].data(), j, f), b = ranges_upper(hi[(size_t)r].data(), j, f);
                if (p == 0 && (bits(a) != bits(lo[(size_t)r][(size_t)i]) || bits(b) != bits(hi[(size_t)r][(size_t)i]))) {
                    fprintf(stderr, "f=%d U=%d: phase 0 of column %d is not the source's bits\n", f, U, j);
                    return 1;
                }
                olo[(size_t)r * Ud + j] = a;
                ohi[(size_t)r * Ud + j] = b;
            }
        fwrite(olo.data(), sizeof(float), olo.size(), out);
        fwrite(ohi.data(), sizeof(float), ohi.size(), out);
        cases++;
    }
    fclose(in);
    fclose(out);
    printf("ranges rule: %d cases ok\n", cases);
    return 0;
}
