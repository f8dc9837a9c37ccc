// The view warp through the C++11 host wrapper (include/rslf_hip.hpp): rslfx::Depth2DComputer::get_warped_view /
// get_view_prediction (through rslf_view_warp_host) and the same getters of a kept rslfx::FineToCoarse (through
// rslf_f2c_run_view_warp_host).  Built with g++ -std=c++11 against librslf_hip.so.  Reads <dir>/input.f32, a synthetic field
// [40][7][96] in [0, 1); runs the classes and writes the planes they read and the planes they return for the pytest side
// (tests/test_gpu_cpp_view_warp.py), which holds them to the numpy yardstick.  Here: the getters' refusals, an object built
// on a MultiContext, and that the calls leave the objects' own planes alone.
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

static void dump_all(const std::string& stem, const rslfx::Warp& w)
{
    dump(stem + "_hit.u8", w.hit);
    dump(stem + "_depth.f32", w.depth);
    dump(stem + "_src_view.i32", w.src_view);
    dump(stem + "_src_col.i32", w.src_col);
    dump(stem + "_count.i32", w.count);
    dump(stem + "_colour.f32", w.colour);
}

static void dump_all(const std::string& stem, const rslfx::ViewPrediction& p)
{
    dump(stem + "_err.f32", p.err);
    dump(stem + "_hit.u8", p.hit);
    dump(stem + "_row_err.f64", p.row_err);
    dump(stem + "_row_hits.i32", p.row_hits);
    dump(stem + "_mean_abs_error.f64", p.mean_abs_error);
    dump(stem + "_coverage.f64", p.coverage);
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

static bool same(const rslfx::Warp& a, const rslfx::Warp& b)
{
    return same_bytes(a.hit, b.hit) && same_bytes(a.depth, b.depth) && same_bytes(a.src_view, b.src_view) && same_bytes(a.src_col, b.src_col) &&
           same_bytes(a.count, b.count) && same_bytes(a.colour, b.colour);
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
    if (!refuses([&] { (void)comp.get_warped_view(3.0f); }) || !refuses([&] { (void)comp.get_view_prediction(); }))   // before run()
        rc |= 1;
    comp.run();
    const std::vector<float> depth = comp.get_depths_s_v_u();
    const std::vector<uint8_t> mask = comp.get_valid_depths_mask_s_v_u();
    const rslfx::Warp centre = comp.get_warped_view(3.0f, 3);   // the centre view from the six others, the object's own mask
    if (centre.hit.size() != row || centre.colour.size() != row || centre.count.size() != row)
        rc |= 2;
    if (!same(centre, comp.get_warped_view(ctx, 3.0f, 3, 0, 1, mask.data(), true)))   // the defaults, named
        rc |= 4;
    std::vector<uint8_t> own(n);
    for (size_t i = 0; i < n; i++)
        own[i] = i % 5 ? 255 : 0;
    const rslfx::Warp between = comp.get_warped_view(2.5f, -1, 2, -1, own.data(), false);
    if (!between.colour.empty() || same_bytes(between.hit, centre.hit) || !same_bytes(comp.get_depths_s_v_u(), depth) ||
        !same_bytes(comp.get_valid_depths_mask_s_v_u(), mask))
        rc |= 8;
    if (!refuses([&] { (void)comp.get_warped_view(std::nanf("")); }) || !refuses([&] { (void)comp.get_warped_view(1e9f); }) ||
        !refuses([&] { (void)comp.get_warped_view(3.0f, -1, 0, 0); }))   // a NaN target, one beyond 65536, nearer = 0
        rc |= 16;
    const rslfx::ViewPrediction all = comp.get_view_prediction();
    std::vector<int> two;
    two.push_back(1), two.push_back(5);
    const rslfx::ViewPrediction picked = comp.get_view_prediction(two, 3, 1, own.data());
    if (all.err.size() != n || all.mean_abs_error.size() != (size_t)S || picked.err.size() != 2 * row || picked.coverage.size() != 2)
        rc |= 16;
    if (!refuses([&] { (void)comp.get_view_prediction(std::vector<int>(1, S)); }))   // not a view
        rc |= 16;
    dump(dir + "/sweep_depth.f32", depth);
    dump(dir + "/sweep_mask.u8", mask);
    dump(dir + "/sweep_own_mask.u8", own);
    dump_all(dir + "/sweep_centre", centre);
    dump_all(dir + "/sweep_between", between);
    dump_all(dir + "/sweep_all", all);
    dump_all(dir + "/sweep_picked", picked);
    // an object built on a MultiContext: the same sweep, bit for bit; the getter takes the Context to run on, and holds no volume
    Sweep shared(multi, epis.data(), false, V, S, U, 0, -2.0f, 2.0f, D, 1.0f);
    shared.run();
    if (!refuses([&] { (void)shared.get_warped_view(3.0f, 3, 0, 1, nullptr, false); }) || !refuses([&] { (void)shared.get_warped_view(ctx, 3.0f, 3); }) ||
        !refuses([&] { (void)shared.get_view_prediction(ctx); }))
        rc |= 32;
    const rslfx::Warp bare = shared.get_warped_view(ctx, 3.0f, 3, 0, 1, nullptr, false);
    if (!same_bytes(shared.get_depths_s_v_u(), depth) || !same_bytes(bare.hit, centre.hit) || !same_bytes(bare.depth, centre.depth) ||
        !same_bytes(bare.src_col, centre.src_col) || !bare.colour.empty())
        rc |= 64;

    // ---- FineToCoarse, a kept run --------------------------------------------------------------------------------------------
    rslfx::Depth1DParameters params;
    F2c f2c(ctx, epis.data(), rslfx::InputType::F32, V, S, U, 0, -2.0f, 2.0f, D, 1.0f, params);
    if (!refuses([&] { (void)f2c.get_warped_view(3.0f); }) || !refuses([&] { (void)f2c.get_view_prediction(); }))   // not a kept run
        rc |= 128;
    f2c.keep_on_device(true);
    f2c.run();
    if (f2c.pyramid_depth() != 2)
        rc |= 256;
    std::vector<float> map;
    std::vector<uint8_t> valid;
    f2c.get_results(map, valid);
    const rslfx::Warp fused = f2c.get_warped_view(3.0f, 0, true, 3);
    const rslfx::Warp level1 = f2c.get_warped_view(3.5f, 1, false, -1, 2, 1, true);
    const rslfx::ViewPrediction pred = f2c.get_view_prediction();
    const size_t row1 = (size_t)f2c.pyramid_dims()[1].first * f2c.pyramid_dims()[1].second;
    if (fused.hit.size() != row || fused.colour.size() != row || level1.hit.size() != row1 || pred.err.size() != n)
        rc |= 512;
    if (!refuses([&] { (void)f2c.get_warped_view(3.0f, 1); }) || !refuses([&] { (void)f2c.get_warped_view(3.0f, 2, false); }) ||
        !refuses([&] { (void)f2c.get_view_prediction(-1, false); }))   // the fused planes are level 0's; levels 2 and -1 do not exist
        rc |= 1024;
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
    dump_all(dir + "/f2c_pred", pred);
    // a run kept without its volumes: the geometry planes only
    F2c lean(ctx, epis.data(), rslfx::InputType::F32, V, S, U, 0, -2.0f, 2.0f, D, 1.0f, params);
    lean.keep_on_device(false);
    lean.run();
    if (!refuses([&] { (void)lean.get_warped_view(3.0f, 0, true, 3); }) || !refuses([&] { (void)lean.get_view_prediction(); }))
        rc |= 4096;
    const rslfx::Warp lean_fused = lean.get_warped_view(3.0f, 0, true, 3, 0, 1, false);
    if (!same_bytes(lean_fused.hit, fused.hit) || !same_bytes(lean_fused.src_view, fused.src_view) || !lean_fused.colour.empty())
        rc |= 8192;
    F2c on_multi(multi, epis.data(), rslfx::InputType::F32, V, S, U, 0, -2.0f, 2.0f, D, 1.0f, params);
    if (!refuses([&] { (void)on_multi.get_warped_view(ctx, 3.0f); }))   // no kept run on a MultiContext
        rc |= 16384;
    return rc;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    try {
        const int rc = run(dir);
        std::printf("host view warp: %s (0x%x)\n", rc ? "FAILED" : "ok", rc);
        return rc ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 3;
    }
}
