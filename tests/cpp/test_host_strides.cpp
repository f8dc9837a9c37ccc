// The pointer-form constructors of include/rslf_hip.hpp with a non-zero row_stride_bytes: every EPI is a window of a wider
// parent buffer (an ROI Mat's data and step) whose other columns hold poison -- float 3.0e38 in even columns and NaN in odd
// ones, uchar 255 on the left and 0 on the right -- which would show in the scale or in the planes if it were read.
// Writes the window values (dense) and the result planes to <out_dir>/ for the pytest side (tests/test_gpu_cpp_host.py) to
// compare with the oracle.  Built with g++ -std=c++11 against librslf_hip.so, as test_host_wrapper.cpp is.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "rslf_hip.hpp"

template <typename T>
static void dump(const std::string& path, const std::vector<T>& v)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        std::perror(path.c_str());
        std::exit(2);
    }
    std::fclose(f);
}

static void poison(float* row, int from, int to)
{
    for (int k = from; k < to; k++)
        row[k] = (k & 1) ? std::numeric_limits<float>::quiet_NaN() : 3.0e38f;
}
static void poison(unsigned char* row, int from, int to, bool left)
{
    for (int k = from; k < to; k++)
        row[k] = left ? 255 : 0;
}

// V EPIs of S x U x C values, each a window [left, left + U) of its own parent of S x (left + U + right) pixels: the same
// texture in every view, moved by `shift` columns per view on the lower half of the scanlines and brighter there.
template <typename T>
struct Windows {
    std::vector<std::vector<T> > parents;
    std::vector<const void*> ptrs;
    size_t stride;            // bytes between the rows of a window: the parent's row
    std::vector<float> flat;  // the window values, dense [V][S][U][C]

    Windows(int V, int S, int U, int C, int left, int right, unsigned seed) : parents(V), ptrs(V)
    {
        const int W = left + U + right;
        stride = (size_t)W * C * sizeof(T);
        unsigned state = seed;
        for (int v = 0; v < V; v++) {
            std::vector<float> tex((size_t)(U + 2 * S) * C);
            for (size_t i = 0; i < tex.size(); i++) {
                state = state * 1664525u + 1013904223u;
                tex[i] = (float)((state >> 8) & 0xffffu) / 65535.0f;
            }
            parents[v].resize((size_t)S * W * C);
            for (int s = 0; s < S; s++) {
                T* row = parents[v].data() + (size_t)s * W * C;
                fill_padding(row, left * C, (left + U) * C, W * C);
                for (int u = 0; u < U; u++)
                    for (int c = 0; c < C; c++) {
                        const float t = tex[(size_t)(u + S + ((v >= V / 2) ? (s - S / 2) : 0)) * C + c];
                        const T x = value(t, v >= V / 2);
                        row[(size_t)(left + u) * C + c] = x;
                        flat.push_back((float)x);
                    }
            }
            ptrs[v] = parents[v].data() + (size_t)left * C;
        }
    }

private:
    static void fill_padding(float* row, int a, int b, int n) { poison(row, 0, a), poison(row, b, n); }
    static void fill_padding(unsigned char* row, int a, int b, int n) { poison(row, 0, a, true), poison(row, b, n, false); }
    static float value(float t, bool bright, float*) { return 3.0f + (bright ? 170.0f : 60.0f) * t; }
    static unsigned char value(float t, bool bright, unsigned char*) { return (unsigned char)std::floor((bright ? 250.0f : 120.0f) * t); }
    static T value(float t, bool bright) { return value(t, bright, (T*)nullptr); }
};

template <class Computer>
static void dump_pile(const std::string& dir, const std::string& tag, const std::vector<float>& input, const Computer& c)
{
    dump(dir + "/" + tag + "_input.f32", input);
    dump(dir + "/" + tag + "_Ce.f32", c.m_edge_confidence_v_u);
    dump(dir + "/" + tag + "_mask.u8", c.m_edge_confidence_mask_v_u);
    dump(dir + "/" + tag + "_Cd.f32", c.m_disp_confidence_v_u);
    dump(dir + "/" + tag + "_depth.f32", c.m_best_depth_v_u);
    dump(dir + "/" + tag + "_rbar.f32", c.m_rbar_v_u);
    dump(dir + "/" + tag + "_idx.i32", c.m_depth_idx_v_u);
    dump(dir + "/" + tag + "_score.f32", c.m_score_v_u);
    dump(dir + "/" + tag + "_scale.f32", std::vector<float>(1, c.epi_scale_factor()));
    std::printf("%s: scale %.9g, %lld px scanned, kernel %d\n", tag.c_str(), c.epi_scale_factor(), (long long)c.stats.pixels_scanned,
                c.stats.scan_kernel);
}

template <class Computer>
static void dump_sweep(const std::string& dir, const std::string& tag, Computer& c)
{
    dump(dir + "/" + tag + "_depth.f32", c.get_depths_s_v_u());
    dump(dir + "/" + tag + "_mask.u8", c.m_edge_confidence_mask_s_v_u);
    dump(dir + "/" + tag + "_Ce.f32", c.m_edge_confidence_s_v_u);
    dump(dir + "/" + tag + "_Cd.f32", c.m_disp_confidence_s_v_u);
    dump(dir + "/" + tag + "_rbar.f32", c.m_rbar_s_v_u);
    std::printf("%s: %lld px scanned\n", tag.c_str(), (long long)c.stats.pixels_scanned);
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    try {
        rslfx::Context ctx(0);
        {   // Depth1DComputer_pile on a Context: float, one column of padding on the right (a stride that is no multiple of 16)
            const int V = 7, S = 13, U = 150;
            Windows<float> w(V, S, U, 1, 0, 1, 101u);
            rslfx::Depth1DComputer_pile<1> c(ctx, w.ptrs.data(), false, V, S, U, w.stride, -1.5f, 2.0f, 20);
            c.run();
            dump_pile(dir, "pile_f32", w.flat, c);
        }
        {   // ... uchar RGB, 16 pixels either side
            const int V = 7, S = 13, U = 150;
            Windows<unsigned char> w(V, S, U, 3, 16, 16, 102u);
            rslfx::Depth1DComputer_pile<3> c(ctx, w.ptrs.data(), true, V, S, U, w.stride, -1.5f, 2.0f, 20);
            c.run();
            dump_pile(dir, "pile_u8", w.flat, c);
        }
        {   // Depth1DComputer_pile on a MultiContext, two workers: 23 scanlines in chunks of 2 (at most 6 EPIs with the halo:
            // direct per-EPI 2-D copies), float RGB in parents twice as wide
            const int V = 23, S = 9, U = 70;
            Windows<float> w(V, S, U, 3, U / 2, U - U / 2, 103u);
            rslfx::MultiContext multi(std::vector<int>(2, 0));
            multi.set_chunk_rows(2);
            rslfx::Depth1DComputer_pile<3> c(multi, w.ptrs.data(), false, V, S, U, w.stride, -1.0f, 2.0f, 12);
            c.run();
            dump_pile(dir, "multi_f32", w.flat, c);
        }
        {   // ... 40 scanlines in chunks of 12 (more than 8 EPIs a chunk: the pinned gather), uchar with one byte of padding
            const int V = 40, S = 9, U = 70;
            Windows<unsigned char> w(V, S, U, 1, 0, 1, 104u);
            rslfx::MultiContext multi(std::vector<int>(2, 0));
            multi.set_chunk_rows(12);
            rslfx::Depth1DComputer_pile<1> c(multi, w.ptrs.data(), true, V, S, U, w.stride, -1.0f, 2.0f, 12);
            c.run();
            dump_pile(dir, "multi_u8", w.flat, c);
        }
        {   // Depth2DComputer on a Context and on a MultiContext (three workers), FineToCoarse on a Context: one float field,
            // its parents padded differently for each
            const int V = 44, S = 5, U = 64, D = 9;
            Windows<float> a(V, S, U, 1, U / 2, U - U / 2, 105u), b(V, S, U, 1, 0, 1, 105u), c(V, S, U, 1, 16, 16, 105u);
            if (a.flat != b.flat || a.flat != c.flat)
                return 5;
            dump(dir + "/sweep_input.f32", a.flat);
            rslfx::Depth2DComputer<1> d2(ctx, a.ptrs.data(), false, V, S, U, a.stride, -1.0f, 1.0f, D);
            d2.run();
            dump_sweep(dir, "d2", d2);
            rslfx::MultiContext multi(std::vector<int>(3, 0));
            rslfx::Depth2DComputer<1> d2m(multi, b.ptrs.data(), false, V, S, U, b.stride, -1.0f, 1.0f, D);
            d2m.run();
            dump_sweep(dir, "d2m", d2m);
            rslfx::FineToCoarse<1> f2c(ctx, c.ptrs.data(), false, V, S, U, c.stride, -1.0f, 1.0f, D);
            f2c.run();
            std::vector<float> map;
            std::vector<uint8_t> valid;
            f2c.get_results(map, valid);
            dump(dir + "/f2c_map.f32", map);
            dump(dir + "/f2c_valid.u8", valid);
            std::printf("f2c: %d levels, %lld px scanned\n", f2c.pyramid_depth(), (long long)f2c.stats.pixels_scanned);
        }
        // a stride shorter than a row is refused by the constructor (one context) or by run() (MultiContext)
        int refused = 0;
        {
            const int V = 40, S = 9, U = 70;
            Windows<unsigned char> w(V, S, U, 1, 0, 1, 106u);
            try {
                rslfx::Depth1DComputer_pile<1> bad(ctx, w.ptrs.data(), true, V, S, U, (size_t)U - 1, -1.0f, 2.0f, 12);
            } catch (const rslfx::Error& err) {
                refused += err.status == RSLF_ERR_INVALID_ARG;
            }
            rslfx::MultiContext multi(std::vector<int>(2, 0));
            multi.set_chunk_rows(12);
            try {
                rslfx::Depth1DComputer_pile<1> bad(multi, w.ptrs.data(), true, V, S, U, (size_t)U - 1, -1.0f, 2.0f, 12);
                bad.run();
            } catch (const rslfx::Error& err) {
                refused += err.status == RSLF_ERR_INVALID_ARG;
            }
        }
        if (refused != 2) {
            std::fprintf(stderr, "a short row stride was refused %d times of 2\n", refused);
            return 4;
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 3;
    }
}
