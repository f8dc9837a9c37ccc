// The cross-view consistency check through the C++11 host wrapper (include/rslf_hip.hpp): rslfx::Depth2DComputer::
// get_consistency (through rslf_view_consistency_host) and the same getter of a kept rslfx::FineToCoarse (through
// rslf_f2c_run_consistency_host).  Built with g++ -std=c++11 against librslf_hip.so.  Reads <dir>/input.f32, a synthetic
// field [40][7][96] in [0, 1); runs the classes and writes the planes they read and the planes they return for the pytest side
// (tests/test_gpu_cpp_consistency.py), which holds them to the numpy yardstick.  Here: the getters' refusals, an object built
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

static void dump_all(const std::string& stem, const rslfx::Consistency& c)
{
    dump(stem + "_seen.i32", c.seen);
    dump(stem + "_agree.i32", c.agree);
    dump(stem + "_above.i32", c.above);
    dump(stem + "_below.i32", c.below);
    dump(stem + "_fused.f32", c.fused);
    dump(stem + "_valid.u8", c.valid);
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

static bool same(const rslfx::Consistency& a, const rslfx::Consistency& b)
{
    return same_bytes(a.seen, b.seen) && same_bytes(a.agree, b.agree) && same_bytes(a.above, b.above) && same_bytes(a.below, b.below) &&
           same_bytes(a.fused, b.fused) && same_bytes(a.valid, b.valid);
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
    const size_t n = (size_t)S * V * U;
    const std::vector<float> raw = load(dir + "/input.f32", n);
    std::vector<const void*> epis(V);
    for (int v = 0; v < V; v++)
        epis[v] = raw.data() + (size_t)v * S * U;
    rslfx::Context ctx(0);
    rslfx::MultiContext multi(std::vector<int>(1, 0));
    int rc = 0;

    // ---- Depth2DComputer --------------------------------------------------------------------------------------------------
    Sweep comp(ctx, epis.data(), false, V, S, U, 0, -2.0f, 2.0f, D, 1.0f);
    if (!refuses([&] { (void)comp.get_consistency(); }) || !refuses([&] { (void)comp.get_valid_depths_mask_s_v_u(); }))   // before run()
        rc |= 1;
    comp.run();
    const std::vector<float> depth = comp.get_depths_s_v_u();
    const std::vector<uint8_t> mask = comp.get_valid_depths_mask_s_v_u();
    const rslfx::Consistency plain = comp.get_consistency();   // one grid step, every view, the object's own mask
    if (plain.seen.size() != n || plain.valid.size() != n || plain.fused.size() != n)
        rc |= 2;
    if (!same(plain, comp.get_consistency(ctx, 0.25f, 0, 0, mask.data())))   // the defaults, named
        rc |= 4;
    std::vector<uint8_t> own(n);
    for (size_t i = 0; i < n; i++)
        own[i] = i % 5 ? 255 : 0;
    const rslfx::Consistency picked = comp.get_consistency(0.3f, 2, 3, own.data());
    if (same(picked, plain) || !same_bytes(comp.get_depths_s_v_u(), depth) || !same_bytes(comp.get_valid_depths_mask_s_v_u(), mask))
        rc |= 8;
    if (!refuses([&] { (void)comp.get_consistency(std::nanf(""), 0, 0); }))   // a NaN tolerance
        rc |= 16;
    if (!refuses([&] { (void)comp.get_consistency(0.1f, 0, -1); }))
        rc |= 16;
    dump(dir + "/sweep_depth.f32", depth);
    dump(dir + "/sweep_mask.u8", mask);
    dump(dir + "/sweep_own_mask.u8", own);
    dump_all(dir + "/sweep_plain", plain);
    dump_all(dir + "/sweep_picked", picked);
    // an object built on a MultiContext: the same sweep, bit for bit, and the getter takes the Context to run on
    Sweep shared(multi, epis.data(), false, V, S, U, 0, -2.0f, 2.0f, D, 1.0f);
    shared.run();
    if (!refuses([&] { (void)shared.get_consistency(); }))
        rc |= 32;
    if (!same_bytes(shared.get_depths_s_v_u(), depth) || !same(shared.get_consistency(ctx), plain))
        rc |= 64;

    // ---- FineToCoarse, a kept run --------------------------------------------------------------------------------------------
    rslfx::Depth1DParameters params;
    F2c f2c(ctx, epis.data(), rslfx::InputType::F32, V, S, U, 0, -2.0f, 2.0f, D, 1.0f, params);
    if (!refuses([&] { (void)f2c.get_consistency(); }))   // not a kept run
        rc |= 128;
    f2c.keep_on_device(false);
    f2c.run();
    if (f2c.pyramid_depth() != 2)
        rc |= 256;
    std::vector<float> map;
    std::vector<uint8_t> valid;
    f2c.get_results(map, valid);
    const rslfx::Consistency fused = f2c.get_consistency();
    const rslfx::Consistency level1 = f2c.get_consistency(1, false, 0.2f, 2, 1);
    if (fused.seen.size() != n || level1.seen.size() != (size_t)S * f2c.pyramid_dims()[1].first * f2c.pyramid_dims()[1].second)
        rc |= 512;
    if (!refuses([&] { (void)f2c.get_consistency(1); }) || !refuses([&] { (void)f2c.get_consistency(2, false); }) ||
        !refuses([&] { (void)f2c.get_consistency(-1, false); }))   // the fused planes are level 0's; levels 2 and -1 do not exist
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
    F2c on_multi(multi, epis.data(), rslfx::InputType::F32, V, S, U, 0, -2.0f, 2.0f, D, 1.0f, params);
    if (!refuses([&] { (void)on_multi.get_consistency(ctx); }))   // no kept run on a MultiContext
        rc |= 4096;
    return rc;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    try {
        const int rc = run(dir);
        std::printf("host consistency: %s (0x%x)\n", rc ? "FAILED" : "ok", rc);
        return rc ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 3;
    }
}
