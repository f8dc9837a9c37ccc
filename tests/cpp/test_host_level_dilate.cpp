// The level dilation of the pyramid through the C++11 host wrapper (include/rslf_hip.hpp): rslfx::FineToCoarse<1> after
// set_level_dilation(2, RSLF_DILATE_CUBIC), as a kept run, as a run with its levels out and as a plain run, the throw on an
// object built on a MultiContext, and set_u_dilation, which still throws.  Built with g++ -std=c++11 against librslf_hip.so.
// Reads <dir>/input.f32, a synthetic field [44][5][64], and the planes rslf_f2c_run_host_dl computed
// (tests/test_gpu_cpp_level_dilate.py wrote them): every plane must hold the same bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "rslf_hip.hpp"

typedef rslfx::FineToCoarse<1> F2c;

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

template <typename Fn>
static bool refuses(Fn fn)
{
    try {
        fn();
    } catch (const std::invalid_argument&) {
        return true;
    } catch (const std::runtime_error&) {
        return true;
    }
    return false;
}

static std::string level_file(const std::string& dir, const char* name, int level, const char* ext)
{
    return dir + "/" + name + "_" + std::to_string(level) + "." + ext;
}

static int run(const std::string& dir)
{
    const int V = 44, S = 5, U = 64, D = 9, P = 3, F = 2;
    const int dims_v[P] = {44, 22, 11}, dims_u[P] = {64, 32, 16};
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
        EXPECT(f2c.get_level_dilation() == 1 && f2c.get_level_dilation_kind() == RSLF_DILATE_CUBIC);
        EXPECT(throws_invalid([&] { f2c.set_level_dilation(0); }) && throws_invalid([&] { f2c.set_level_dilation(9); }));
        EXPECT(throws_invalid([&] { f2c.set_level_dilation(2, 3); }));
        EXPECT(f2c.get_level_dilation() == 1);
        EXPECT(throws_invalid([&] { f2c.set_u_dilation(2); }));   // the dilation of the level chain is still not built
        f2c.set_u_dilation(1);
        f2c.keep_on_device();
        f2c.set_level_dilation(F, RSLF_DILATE_CUBIC);
        EXPECT(f2c.get_level_dilation() == F && f2c.get_level_dilation_kind() == RSLF_DILATE_CUBIC);
        f2c.run();
        EXPECT(f2c.pyramid_depth() == P);
        f2c.get_results(map, valid);
        EXPECT(same_bytes(map, want_map) && same_bytes(valid, want_valid));
        for (int l = 0; l < P; l++) {
            const size_t n = (size_t)S * dims_v[l] * dims_u[l];   // every plane on the level's own grid
            EXPECT(f2c.pyramid_dims()[l].first == dims_v[l] && f2c.pyramid_dims()[l].second == dims_u[l]);
            EXPECT(same_bytes(f2c.get_depths_pyr()[l], load<float>(level_file(dir, "depth", l, "f32"), n)));
            EXPECT(same_bytes(f2c.get_validity_pyr()[l], load<uint8_t>(level_file(dir, "valid", l, "u8"), n)));
            EXPECT(same_bytes(f2c.get_disp_confidence_pyr()[l], load<float>(level_file(dir, "Cd", l, "f32"), n)));
        }
    }
    // ---- every level's planes out, and the plain run ----------------------------------------------------------------------------
    {
        F2c f2c(ctx, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
        f2c.set_line_confidence_mode(RSLF_LINE_CONF_OFF);
        f2c.set_level_dilation(F);
        f2c.run();
        f2c.get_results(map, valid);
        EXPECT(same_bytes(map, want_map) && same_bytes(valid, want_valid));
        for (int l = 0; l < P; l++) {
            const size_t n = (size_t)S * dims_v[l] * dims_u[l];
            EXPECT(same_bytes(f2c.get_depths_pyr()[l], load<float>(level_file(dir, "depth", l, "f32"), n)));
            EXPECT(same_bytes(f2c.get_validity_pyr()[l], load<uint8_t>(level_file(dir, "valid", l, "u8"), n)));
        }
        // a line-confidence mode together with the dilation: run() reports the library's refusal
        F2c with_lc(ctx, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
        with_lc.set_line_confidence_mode(RSLF_LINE_CONF_AS_BUILT);
        with_lc.set_level_dilation(F);
        EXPECT(refuses([&] { with_lc.run(); }));
        F2c plain(ctx, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
        plain.set_level_dilation(F, RSLF_DILATE_CUBIC);
        plain.run();
        plain.get_results(map, valid);
        EXPECT(same_bytes(map, want_map) && same_bytes(valid, want_valid));
        // 1 switches it off: another result (the undilated pyramid's)
        plain.set_level_dilation(1);
        plain.run();
        plain.get_results(map, valid);
        EXPECT(map.size() == n0 && !same_bytes(map, want_map));
    }
    // ---- the throwing form --------------------------------------------------------------------------------------------------------
    {
        rslfx::MultiContext multi(std::vector<int>(1, 0));
        F2c on_multi(multi, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
        EXPECT(throws_invalid([&] { on_multi.set_level_dilation(F); }));
        EXPECT(on_multi.get_level_dilation() == 1);
        on_multi.set_level_dilation(1);   // nothing to do
        EXPECT(throws_invalid([&] { on_multi.set_u_dilation(2); }));
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
        std::printf(rc ? "host level dilate: FAILED\n" : "host level dilate: ok\n");
        return rc;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 3;
    }
}
