// The derivative channels through the C++11 host wrapper (include/rslf_hip.hpp): rslfx::FineToCoarse<1> after
// set_derivative_channels(w), as a kept run, as a run with its levels out and as a plain run, and the two forms that throw --
// an RGB field and an object built on a MultiContext.  Built with g++ -std=c++11 against librslf_hip.so.  Reads
// <dir>/input.f32, a synthetic field [44][5][44] in [0, 1), and the planes the Python call
// fine_to_coarse_run_host(..., keep=True, derivative_channels=1.5) computed (tests/test_gpu_cpp_derivative.py wrote them):
// every plane must hold the same bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "rslf_hip.hpp"

typedef rslfx::FineToCoarse<1> F2c;
typedef rslfx::FineToCoarse<3> F2cRgb;

template <typename T>
static std::vector<T> load(const std::string& path, size_t n)
{
    std::vector<T> v(n);
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f || std::fread(v.data(), sizeof(T), n, f) != n) {
        std::perror(path.c_str());
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

template <typename T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

template <typename Fn>
static bool throws_invalid(Fn fn)
{
    try {
        fn();
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

#define EXPECT(cond)                                                           \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("%s:%d: EXPECT failed: %s\n", __FILE__, __LINE__, #cond); \
            rc = 1;                                                            \
        }                                                                      \
    } while (0)

static std::string level_file(const std::string& dir, const char* name, int level, const char* ext)
{
    return dir + "/" + name + "_" + std::to_string(level) + "." + ext;
}

static int run(const std::string& dir)
{
    const int V = 44, S = 5, U = 44, D = 10, P = 3;
    const float W = 1.5f;
    const int dims[P] = {44, 22, 11};
    const std::vector<float> raw = load<float>(dir + "/input.f32", (size_t)V * S * U);
    std::vector<const void*> epis(V);
    for (int v = 0; v < V; v++)
        epis[v] = raw.data() + (size_t)v * S * U;
    const size_t n0 = (size_t)S * V * U;
    const std::vector<float> want_map = load<float>(dir + "/fused_map.f32", n0);
    const std::vector<uint8_t> want_valid = load<uint8_t>(dir + "/fused_valid.u8", n0);
    rslfx::Context ctx(0);
    int rc = 0;
    std::vector<float> map;
    std::vector<uint8_t> valid;

    // ---- a kept run ---------------------------------------------------------------------------------------------------------
    {
        F2c f2c(ctx, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
        EXPECT(f2c.get_derivative_channels() == 0.0f);
        EXPECT(throws_invalid([&] { f2c.set_derivative_channels(-1.0f); }));
        EXPECT(f2c.get_derivative_channels() == 0.0f);
        f2c.keep_on_device();
        f2c.set_derivative_channels(W);
        EXPECT(f2c.get_derivative_channels() == W);
        f2c.run();
        EXPECT(f2c.pyramid_depth() == P);
        f2c.get_results(map, valid);
        EXPECT(same_bytes(map, want_map) && same_bytes(valid, want_valid));
        for (int l = 0; l < P; l++) {
            const size_t n = (size_t)S * dims[l] * dims[l];
            EXPECT(f2c.pyramid_dims()[l].first == dims[l] && f2c.pyramid_dims()[l].second == dims[l]);
            EXPECT(same_bytes(f2c.get_depths_pyr()[l], load<float>(level_file(dir, "depth", l, "f32"), n)));
            EXPECT(same_bytes(f2c.get_validity_pyr()[l], load<uint8_t>(level_file(dir, "valid", l, "u8"), n)));
            EXPECT(same_bytes(f2c.get_disp_confidence_pyr()[l], load<float>(level_file(dir, "Cd", l, "f32"), n)));
        }
    }
    // ---- every level's planes out, and the plain run ----------------------------------------------------------------------------
    {
        F2c f2c(ctx, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
        f2c.set_line_confidence_mode(RSLF_LINE_CONF_OFF);
        f2c.set_derivative_channels(W);
        f2c.run();
        f2c.get_results(map, valid);
        EXPECT(same_bytes(map, want_map) && same_bytes(valid, want_valid));
        for (int l = 0; l < P; l++) {
            const size_t n = (size_t)S * dims[l] * dims[l];
            EXPECT(same_bytes(f2c.get_depths_pyr()[l], load<float>(level_file(dir, "depth", l, "f32"), n)));
            EXPECT(same_bytes(f2c.get_validity_pyr()[l], load<uint8_t>(level_file(dir, "valid", l, "u8"), n)));
        }
        F2c plain(ctx, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
        plain.set_derivative_channels(W);
        plain.run();
        plain.get_results(map, valid);
        EXPECT(same_bytes(map, want_map) && same_bytes(valid, want_valid));
        // 0 switches it off: another result (the one-channel pyramid's)
        plain.set_derivative_channels(0.0f);
        plain.run();
        plain.get_results(map, valid);
        EXPECT(map.size() == n0 && !same_bytes(map, want_map));
    }
    // ---- the two throwing forms -------------------------------------------------------------------------------------------------
    {
        const std::vector<float> rgb_raw((size_t)V * S * U * 3, 0.5f);
        std::vector<const void*> rgb(V);
        for (int v = 0; v < V; v++)
            rgb[v] = rgb_raw.data() + (size_t)v * S * U * 3;
        F2cRgb on_rgb(ctx, rgb.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
        EXPECT(throws_invalid([&] { on_rgb.set_derivative_channels(W); }));
        EXPECT(on_rgb.get_derivative_channels() == 0.0f);
        on_rgb.set_derivative_channels(0.0f);   // nothing to do
        rslfx::MultiContext multi(std::vector<int>(1, 0));
        F2c on_multi(multi, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
        EXPECT(throws_invalid([&] { on_multi.set_derivative_channels(W); }));
        EXPECT(on_multi.get_derivative_channels() == 0.0f);
    }
    return rc;
}

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::printf("usage: %s <dir>\n", argv[0]);
        return 2;
    }
    try {
        const int rc = run(argv[1]);
        std::printf(rc ? "host derivative: FAILED\n" : "host derivative: ok\n");
        return rc;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 3;
    }
}
