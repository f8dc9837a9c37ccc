// The per-view equalisation through the C++11 host wrapper (include/rslf_hip.hpp): rslfx::FineToCoarse<1> after
// set_equalize_views(RSLF_EQUALIZE_AFFINE), as a kept run, as a run with its levels out and as a plain run, get_view_gains,
// and the forms that throw -- bad options and an object built on a MultiContext.  Built with g++ -std=c++11 against
// librslf_hip.so.  Reads <dir>/input.f32, a synthetic field [44][5][44] with two drifted views, and the planes and
// coefficients the C entry computed through the Python call fine_to_coarse_run_host(..., keep=True,
// equalize_views=EQUALIZE_AFFINE) (tests/test_gpu_cpp_equalize.py wrote them): every plane must hold the same bytes.
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
    const int dims[P] = {44, 22, 11};
    const std::vector<float> raw = load<float>(dir + "/input.f32", (size_t)V * S * U);
    std::vector<const void*> epis(V);
    for (int v = 0; v < V; v++)
        epis[v] = raw.data() + (size_t)v * S * U;
    const size_t n0 = (size_t)S * V * U;
    const std::vector<float> want_map = load<float>(dir + "/fused_map.f32", n0);
    const std::vector<uint8_t> want_valid = load<uint8_t>(dir + "/fused_valid.u8", n0);
    const std::vector<float> want_gains = load<float>(dir + "/view_gains.f32", (size_t)S * 2);
    const std::vector<float> want_gains_mean = load<float>(dir + "/view_gains_mean.f32", (size_t)S * 2);
    rslfx::Context ctx(0);
    int rc = 0;
    std::vector<float> map;
    std::vector<uint8_t> valid;

    // ---- a kept run ---------------------------------------------------------------------------------------------------------
    {
        F2c f2c(ctx, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
        EXPECT(f2c.get_equalize_views() == 0 && f2c.get_view_gains().empty());
        EXPECT(throws_invalid([&] { f2c.set_equalize_views(3); }));
        EXPECT(throws_invalid([&] { f2c.set_equalize_views(RSLF_EQUALIZE_AFFINE, S); }));
        EXPECT(throws_invalid([&] { f2c.set_equalize_views(RSLF_EQUALIZE_AFFINE, -3); }));
        EXPECT(throws_invalid([&] { f2c.set_equalize_views(RSLF_EQUALIZE_AFFINE, 0, 1); }));          // joint on one channel
        EXPECT(throws_invalid([&] { f2c.set_equalize_views(RSLF_EQUALIZE_GAIN, 0, 0, 0.5f); }));
        EXPECT(f2c.get_equalize_views() == 0);
        f2c.keep_on_device();
        f2c.set_equalize_views(RSLF_EQUALIZE_AFFINE);   // the centre view, max_gain 4
        EXPECT(f2c.get_equalize_views() == RSLF_EQUALIZE_AFFINE);
        f2c.run();
        EXPECT(f2c.pyramid_depth() == P);
        f2c.get_results(map, valid);
        EXPECT(same_bytes(map, want_map) && same_bytes(valid, want_valid));
        EXPECT(same_bytes(f2c.get_view_gains(), want_gains));
        for (int l = 0; l < P; l++) {
            const size_t n = (size_t)S * dims[l] * dims[l];
            EXPECT(f2c.pyramid_dims()[l].first == dims[l] && f2c.pyramid_dims()[l].second == dims[l]);
            EXPECT(same_bytes(f2c.get_depths_pyr()[l], load<float>(level_file(dir, "depth", l, "f32"), n)));
            EXPECT(same_bytes(f2c.get_validity_pyr()[l], load<uint8_t>(level_file(dir, "valid", l, "u8"), n)));
            EXPECT(same_bytes(f2c.get_disp_confidence_pyr()[l], load<float>(level_file(dir, "Cd", l, "f32"), n)));
        }
        // GAIN towards the views' mean with the gain clamped at 2: the C entry's coefficients
        f2c.set_equalize_views(RSLF_EQUALIZE_GAIN, -1, 0, 2.0f);
        f2c.run();
        EXPECT(same_bytes(f2c.get_view_gains(), want_gains_mean));
        // 0 switches it off: a run without coefficients
        f2c.set_equalize_views(0);
        f2c.run();
        EXPECT(f2c.get_view_gains().empty());
        f2c.get_results(map, valid);
        EXPECT(map.size() == n0 && !same_bytes(map, want_map));
    }
    // ---- every level's planes out, and the plain run ----------------------------------------------------------------------------
    {
        F2c f2c(ctx, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
        f2c.set_line_confidence_mode(RSLF_LINE_CONF_OFF);
        f2c.set_equalize_views(RSLF_EQUALIZE_AFFINE, S / 2, 0, 4.0f);
        f2c.run();
        f2c.get_results(map, valid);
        EXPECT(same_bytes(map, want_map) && same_bytes(valid, want_valid));
        for (int l = 0; l < P; l++) {
            const size_t n = (size_t)S * dims[l] * dims[l];
            EXPECT(same_bytes(f2c.get_depths_pyr()[l], load<float>(level_file(dir, "depth", l, "f32"), n)));
            EXPECT(same_bytes(f2c.get_validity_pyr()[l], load<uint8_t>(level_file(dir, "valid", l, "u8"), n)));
        }
        F2c plain(ctx, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
        plain.set_equalize_views(RSLF_EQUALIZE_AFFINE);
        plain.run();
        plain.get_results(map, valid);
        EXPECT(same_bytes(map, want_map) && same_bytes(valid, want_valid));
        EXPECT(plain.get_view_gains().empty());   // (no kept run: the host-planes entries hand no coefficients out)
    }
    // ---- the throwing forms -----------------------------------------------------------------------------------------------------
    {
        const std::vector<float> rgb_raw((size_t)V * S * U * 3, 0.5f);
        std::vector<const void*> rgb(V);
        for (int v = 0; v < V; v++)
            rgb[v] = rgb_raw.data() + (size_t)v * S * U * 3;
        F2cRgb on_rgb(ctx, rgb.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
        on_rgb.set_equalize_views(RSLF_EQUALIZE_GAIN);          // joint by default on three channels
        on_rgb.set_equalize_views(RSLF_EQUALIZE_GAIN, 0, 0);    // and a pair per channel
        rslfx::MultiContext multi(std::vector<int>(1, 0));
        F2c on_multi(multi, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
        EXPECT(throws_invalid([&] { on_multi.set_equalize_views(RSLF_EQUALIZE_AFFINE); }));
        EXPECT(throws_invalid([&] { on_multi.set_equalize_views(RSLF_EQUALIZE_GAIN, -1, 0, 2.0f); }));
        EXPECT(on_multi.get_equalize_views() == 0);
        on_multi.set_equalize_views(0);   // nothing to do
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
        std::printf(rc ? "host equalize: FAILED\n" : "host equalize: ok\n");
        return rc;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 3;
    }
}
