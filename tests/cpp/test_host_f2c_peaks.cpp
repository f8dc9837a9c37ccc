// FineToCoarse of include/rslf_hip.hpp with set_peaks and set_uniqueness_ratio on the field the pytest side hands over
// (tests/test_gpu_cpp_f2c_peaks.py writes <dir>/input.f32, [V][S][U] float32): the setters' refusals, then every peak plane
// and the fused planes against what the C entry rslf_f2c_run_host_pk gives for the same arguments, byte for byte.  Built with
// g++ -std=c++11 against librslf_hip.so.  Writes the fused map, fused_level and level 0's validity to <dir>/ for the pytest
// side, which holds them to tests/f2c_peaks_ref.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
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

template <typename F>
static bool refuses(F call)
{
    try {
        call();
    } catch (const rslfx::Error& e) {
        return e.status == RSLF_ERR_INVALID_ARG;
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

template <typename T>
static bool same(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

template <typename T>
static std::vector<T> copy_plane(const rslf_f2c_run* run, int level, int which, size_t n)
{
    std::vector<T> out(n);
    if (rslf_f2c_run_copy(run, level, which, out.data(), 1, nullptr) != RSLF_OK)
        throw std::runtime_error(std::string("rslf_f2c_run_copy: ") + rslf_last_error());
    return out;
}

typedef rslfx::FineToCoarse<1> F2c;

static bool same_peaks(const F2c::Peaks& p, const rslf_f2c_run* run, int level, int first, size_t n)
{
    return same(p.idx, copy_plane<int32_t>(run, level, first, n)) && same(p.score, copy_plane<float>(run, level, first + 1, n)) &&
           same(p.runner_idx, copy_plane<int32_t>(run, level, first + 2, n)) &&
           same(p.runner_score, copy_plane<float>(run, level, first + 3, n));
}

static int run(const std::string& dir)
{
    const int V = 44, S = 5, U = 64, D = 9;
    const float ratio = 0.7f;
    std::vector<float> flat((size_t)V * S * U);
    FILE* f = std::fopen((dir + "/input.f32").c_str(), "rb");
    if (!f || std::fread(flat.data(), sizeof(float), flat.size(), f) != flat.size())
        return 1;
    std::fclose(f);
    std::vector<const void*> ptrs(V);
    for (int v = 0; v < V; v++)
        ptrs[v] = flat.data() + (size_t)v * S * U;
    rslfx::Context ctx(0);
    rslfx::MultiContext multi(std::vector<int>(1, 0));
    rslfx::Depth1DParameters params;

    // the setters' refusals: without keep_on_device, on several devices, a ratio outside [0, 1], a ratio without peaks
    F2c f2c(ctx, ptrs.data(), rslfx::InputType::F32, V, S, U, 0, -1.0f, 1.0f, D, -1, params);
    if (!refuses([&] { f2c.set_peaks(true); }) || !refuses([&] { f2c.set_uniqueness_ratio(ratio); }))
        return 2;
    F2c on_multi(multi, ptrs.data(), rslfx::InputType::F32, V, S, U, 0, -1.0f, 1.0f, D, -1, params);
    if (!refuses([&] { on_multi.set_peaks(true); }) || !refuses([&] { on_multi.set_uniqueness_ratio(ratio); }))
        return 4;
    f2c.keep_on_device(false);
    if (!refuses([&] { f2c.set_uniqueness_ratio(1.5f); }) || !refuses([&] { f2c.set_uniqueness_ratio(-0.5f); }))
        return 8;
    f2c.set_uniqueness_ratio(ratio);
    if (!refuses([&] { f2c.run(); }))   // the ratio reads the peak planes
        return 16;
    if (!refuses([&] { f2c.get_fused_level(); }))
        return 32;
    f2c.set_peaks(true);
    if (!f2c.get_peaks_mode() || f2c.get_uniqueness_ratio() != ratio)
        return 64;
    f2c.run();

    // the same arguments through the C entry
    const rslf_params p = params.to_c();
    rslf_f2c_run* raw = nullptr;
    rslf_stats st;
    if (rslf_f2c_run_host_pk(ctx.get(), ptrs.data(), RSLF_ELEM_F32, V, S, U, 1, 0, -1.0f, 1.0f, D, -1.0f, &p, -1, 1, RSLF_LINE_CONF_OFF,
                             RSLF_F2C_VALID_COMPAT, 0, &raw, &st, 0, 1, ratio) != RSLF_OK) {
        std::fprintf(stderr, "rslf_f2c_run_host_pk: %s\n", rslf_last_error());
        return 128;
    }
    int rc = 0;
    if (rslf_f2c_run_peaks(raw) != 1 || rslf_f2c_run_uniqueness(raw) != ratio)
        rc |= 256;
    if (f2c.pyramid_depth() != 3 || st.pixels_scanned != f2c.stats.pixels_scanned)
        rc |= 512;
    for (int l = 0; l < f2c.pyramid_depth(); l++) {
        const size_t n = (size_t)S * f2c.pyramid_dims()[l].first * f2c.pyramid_dims()[l].second;
        if (!same_peaks(f2c.get_level_peaks(l), raw, l, RSLF_F2C_PLANE_PK_IDX, n))
            rc |= 1024;
        if (!same(f2c.get_validity_pyr()[l], copy_plane<uint8_t>(raw, l, RSLF_F2C_PLANE_VALID, n)) ||
            !same(f2c.get_depths_pyr()[l], copy_plane<float>(raw, l, RSLF_F2C_PLANE_DEPTH, n)))
            rc |= 2048;
    }
    const size_t n0 = (size_t)S * V * U;
    if (!same_peaks(f2c.get_fused_peaks(), raw, 0, RSLF_F2C_PLANE_FUSED_PK_IDX, n0))
        rc |= 4096;
    const std::vector<uint8_t> level = f2c.get_fused_level();
    if (!same(level, copy_plane<uint8_t>(raw, 0, RSLF_F2C_PLANE_FUSED_LEVEL, n0)))
        rc |= 8192;
    std::vector<float> map;
    std::vector<uint8_t> valid;
    f2c.get_results(map, valid);
    if (!same(map, copy_plane<float>(raw, 0, RSLF_F2C_PLANE_FUSED_MAP, n0)))
        rc |= 16384;
    if (!refuses([&] { f2c.get_level_peaks(3); }))
        rc |= 32768;
    rslf_f2c_run_destroy(raw);
    dump(dir + "/fused_map.f32", map);
    dump(dir + "/fused_level.u8", level);
    dump(dir + "/fused_idx.i32", f2c.get_fused_peaks().idx);
    dump(dir + "/valid0.u8", f2c.get_validity_pyr()[0]);

    // the ratio off again: the fused map is another one, every pixel decided by level 0
    f2c.set_uniqueness_ratio(0.0f);
    f2c.run();
    std::vector<float> map_off;
    f2c.get_results(map_off, valid);
    const std::vector<uint8_t> level_off = f2c.get_fused_level();
    size_t coarse = 0;
    for (size_t i = 0; i < level_off.size(); i++)
        coarse += level_off[i] != 0;
    if (same(map, map_off) || coarse != 0)
        rc |= 65536;
    return rc;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    try {
        const int rc = run(dir);
        std::printf("host f2c peaks: %s (0x%x)\n", rc ? "FAILED" : "ok", rc);
        return rc ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 3;
    }
}
