// The novel view through the C++11 host wrapper (include/rslf_hip.hpp): rslfx::Depth2DComputer::get_novel_view (through
// rslf_novel_view_host) and the same getter of a kept rslfx::FineToCoarse (through rslf_f2c_run_novel_view_host).  Built with
// g++ -std=c++11 against librslf_hip.so.  Reads <dir>/input.f32, a synthetic field [40][7][96] in [0, 1); runs the classes and
// writes the planes they read and the planes they return for the pytest side (tests/test_gpu_cpp_novel_view.py), which holds
// them to the numpy yardstick.  Here: the getters' refusals, an object built on a MultiContext, and that the calls leave the
// objects' own planes alone.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "rslf_hip.hpp"

typedef rslfx::Depth2DComputer<1> Sweep;
typedef rslfx::FineToCoarse<1> F2c;

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

static void dump_all(const std::string& stem, const rslfx::NovelView& w)
{
    dump(stem + "_colour.f32", w.colour);
    dump(stem + "_depth.f32", w.depth);
    dump(stem + "_fill.u8", w.fill);
    dump(stem + "_n_src.i32", w.n_src);
}

static std::vector<float> load(const std::string& path, size_t n)
{
    std::vector<float> v(n);
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f || std::fread(v.data(), sizeof(float), n, f) != n) {
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

static bool same(const rslfx::NovelView& a, const rslfx::NovelView& b)
{
    return same_bytes(a.colour, b.colour) && same_bytes(a.depth, b.depth) && same_bytes(a.fill, b.fill) && same_bytes(a.n_src, b.n_src);
}

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

static rslfx::NovelViewOptions options(int radius, int nearer, int max_gap, int sources, float tol)
{
    rslfx::NovelViewOptions o;
    o.radius = radius, o.nearer = nearer, o.max_gap = max_gap, o.sources = sources, o.tol = tol;
    return o;
}

static int run(const std::string& dir)
{
    const int V = 40, S = 7, U = 96, D = 17;
    const size_t n = (size_t)S * V * U, row = (size_t)V * U;
    const std::vector<float> raw = load(dir + "/input.f32", n);
    std::vector<const void*> epis(V);
    for (int v = 0; v < V; v++)
        epis[v] = raw.data() + (size_t)v * S * U;
    rslfx::Context ctx(0);
    rslfx::MultiContext multi(std::vector<int>(1, 0));
    int rc = 0;

    // ---- Depth2DComputer --------------------------------------------------------------------------------------------------
    Sweep comp(ctx, epis.data(), false, V, S, U, 0, -2.0f, 2.0f, D, 1.0f);
    if (!refuses([&] { (void)comp.get_novel_view(3.0f); }))   // before run()
        rc |= 1;
    comp.run();
    const std::vector<float> depth = comp.get_depths_s_v_u();
    const std::vector<uint8_t> mask = comp.get_valid_depths_mask_s_v_u();
    const rslfx::NovelView centre = comp.get_novel_view(3.0f, 3);   // the centre view from the six others: mask, grid step, 4 sources
    if (centre.fill.size() != row || centre.colour.size() != row || centre.n_src.size() != row || centre.depth.size() != row)
        rc |= 2;
    if (!same(centre, comp.get_novel_view(ctx, 3.0f, 3, options(0, 1, 0, 4, 0.25f), mask.data(), true)))   // the defaults, named
        rc |= 4;
    std::vector<uint8_t> own(n);
    for (size_t i = 0; i < n; i++)
        own[i] = i % 5 ? 255 : 0;
    const rslfx::NovelView between = comp.get_novel_view(2.5f, -1, options(2, -1, 2, 2, 0.5f), own.data(), false);
    if (!between.colour.empty() || same_bytes(between.n_src, centre.n_src) || !same_bytes(comp.get_depths_s_v_u(), depth) ||
        !same_bytes(comp.get_valid_depths_mask_s_v_u(), mask))
        rc |= 8;
    if (!refuses([&] { (void)comp.get_novel_view(std::nanf("")); }) || !refuses([&] { (void)comp.get_novel_view(1e9f); }) ||
        !refuses([&] { (void)comp.get_novel_view(3.0f, -1, options(0, 0, 0, 4, 0.1f)); }) ||    // a NaN target, one beyond 65536, nearer = 0,
        !refuses([&] { (void)comp.get_novel_view(3.0f, -1, options(0, 1, 0, 0, 0.1f)); }) ||    // no source,
        !refuses([&] { (void)comp.get_novel_view(3.0f, -1, options(0, 1, 0, 4, std::nanf(""))); }))   // a tolerance that is none
        rc |= 16;
    dump(dir + "/sweep_depth.f32", depth);
    dump(dir + "/sweep_mask.u8", mask);
    dump(dir + "/sweep_own_mask.u8", own);
    dump_all(dir + "/sweep_centre", centre);
    dump_all(dir + "/sweep_between", between);
    // an object built on a MultiContext: the same sweep, bit for bit; the getter takes the Context to run on, and holds no volume
    Sweep shared(multi, epis.data(), false, V, S, U, 0, -2.0f, 2.0f, D, 1.0f);
    shared.run();
    if (!refuses([&] { (void)shared.get_novel_view(3.0f, 3, rslfx::NovelViewOptions(), nullptr, false); }) ||
        !refuses([&] { (void)shared.get_novel_view(ctx, 3.0f, 3); }))
        rc |= 32;
    const rslfx::NovelView bare = shared.get_novel_view(ctx, 3.0f, 3, rslfx::NovelViewOptions(), nullptr, false);
    if (!same_bytes(shared.get_depths_s_v_u(), depth) || !same_bytes(bare.fill, centre.fill) || !same_bytes(bare.depth, centre.depth) ||
        !same_bytes(bare.n_src, centre.n_src) || !bare.colour.empty())
        rc |= 64;

    // ---- FineToCoarse, a kept run --------------------------------------------------------------------------------------------
    rslfx::Depth1DParameters params;
    F2c f2c(ctx, epis.data(), rslfx::InputType::F32, V, S, U, 0, -2.0f, 2.0f, D, 1.0f, params);
    if (!refuses([&] { (void)f2c.get_novel_view(3.0f); }))   // not a kept run
        rc |= 128;
    f2c.keep_on_device(true);
    f2c.run();
    if (f2c.pyramid_depth() != 2)
        rc |= 256;
    std::vector<float> map;
    std::vector<uint8_t> valid;
    f2c.get_results(map, valid);
    const rslfx::NovelView fused = f2c.get_novel_view(3.0f, 0, true, 3);
    const rslfx::NovelView level1 = f2c.get_novel_view(3.5f, 1, false, -1, options(2, 1, 3, 2, 0.3f), true);
    const size_t row1 = (size_t)f2c.pyramid_dims()[1].first * f2c.pyramid_dims()[1].second;
    if (fused.fill.size() != row || fused.colour.size() != row || level1.fill.size() != row1 || level1.colour.size() != row1)
        rc |= 512;
    if (!refuses([&] { (void)f2c.get_novel_view(3.0f, 1); }) || !refuses([&] { (void)f2c.get_novel_view(3.0f, 2, false); }))
        rc |= 1024;   // the fused planes are level 0's; level 2 does not exist
    std::vector<float> map2;
    std::vector<uint8_t> valid2;
    f2c.get_results(map2, valid2);
    if (!same_bytes(map, map2) || !same_bytes(valid, valid2))
        rc |= 2048;
    dump(dir + "/f2c_fused_map.f32", map);
    dump(dir + "/f2c_fused_valid.u8", valid);
    dump(dir + "/f2c_depth1.f32", f2c.get_depths_pyr()[1]);
    dump(dir + "/f2c_valid1.u8", f2c.get_validity_pyr()[1]);
    dump_all(dir + "/f2c_fused", fused);
    dump_all(dir + "/f2c_level1", level1);
    // a run kept without its volumes: the geometry planes only
    F2c lean(ctx, epis.data(), rslfx::InputType::F32, V, S, U, 0, -2.0f, 2.0f, D, 1.0f, params);
    lean.keep_on_device(false);
    lean.run();
    if (!refuses([&] { (void)lean.get_novel_view(3.0f, 0, true, 3); }))
        rc |= 4096;
    const rslfx::NovelView lean_fused = lean.get_novel_view(3.0f, 0, true, 3, rslfx::NovelViewOptions(), false);
    if (!same_bytes(lean_fused.fill, fused.fill) || !same_bytes(lean_fused.n_src, fused.n_src) || !lean_fused.colour.empty())
        rc |= 8192;
    F2c on_multi(multi, epis.data(), rslfx::InputType::F32, V, S, U, 0, -2.0f, 2.0f, D, 1.0f, params);
    if (!refuses([&] { (void)on_multi.get_novel_view(ctx, 3.0f); }))   // no kept run on a MultiContext
        rc |= 16384;
    return rc;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    try {
        const int rc = run(dir);
        std::printf("host novel view: %s (0x%x)\n", rc ? "FAILED" : "ok", rc);
        return rc ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 3;
    }
}
