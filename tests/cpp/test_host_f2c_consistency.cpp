// A kept fine-to-coarse run's validity by cross-view consistency through the C++11 host wrapper (include/rslf_hip.hpp):
// rslfx::FineToCoarse::set_consistency_gate, get_inconsistent and get_gate_counts (through rslf_f2c_run_host_cs).  Built with
// g++ -std=c++11 against librslf_hip.so.  Reads <dir>/input.f32, a synthetic field [40][7][96] in [0, 1); runs the class with
// the gate off and on and writes the planes beside its results for the pytest side (tests/test_gpu_cpp_f2c_consistency.py),
// which holds them to the numpy yardstick.  Here: the setter's refusals, an object built on a MultiContext, the getters
// before and without a gated run, and that the gate off changes nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "rslf_hip.hpp"

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

// one gated run: its planes under <dir>/<stem>_*
static int gated_run(const std::string& dir, const std::string& stem, rslfx::Context& ctx, const void* const* epis, int V, int S, int U, int D,
                     int min_agree, float tol, int radius, const std::vector<float>& depth0_off)
{
    int rc = 0;
    rslfx::Depth1DParameters params;
    F2c f2c(ctx, epis, rslfx::InputType::F32, V, S, U, 0, -2.0f, 2.0f, D, 1.0f, params);
    f2c.keep_on_device(false);
    if (tol < 0.f)
        f2c.set_consistency_gate(min_agree);   // tol: one grid step; every view
    else
        f2c.set_consistency_gate(min_agree, tol, radius);
    if (f2c.get_consistency_min_agree() != min_agree)
        rc |= 1;
    f2c.run();
    if (f2c.pyramid_depth() != 2)
        rc |= 2;
    const size_t n = (size_t)S * V * U;
    const rslfx::Consistency counts = f2c.get_gate_counts(0);
    if (counts.agree.size() != n || counts.seen.size() != n || !counts.fused.empty() || !counts.valid.empty() || !counts.above.empty())
        rc |= 4;
    if (!refuses([&] { (void)f2c.get_gate_counts(1); }))     // the last level is accepted whole: it holds no gate planes
        rc |= 8;
    if (!refuses([&] { (void)f2c.get_gate_counts(2); }) || !refuses([&] { (void)f2c.get_inconsistent(2); }) ||
        !refuses([&] { (void)f2c.get_inconsistent(-1); }))
        rc |= 16;
    if (f2c.get_inconsistent(1) != 0 || f2c.get_inconsistent(0) == 0)
        rc |= 32;
    if (!same_bytes(f2c.get_depths_pyr()[0], depth0_off))   // level 0's sweep never sees the gate
        rc |= 64;
    std::vector<float> map;
    std::vector<uint8_t> valid;
    f2c.get_results(map, valid);
    dump(dir + "/" + stem + "_depth0.f32", f2c.get_depths_pyr()[0]);
    dump(dir + "/" + stem + "_valid0.u8", f2c.get_validity_pyr()[0]);
    dump(dir + "/" + stem + "_depth1.f32", f2c.get_depths_pyr()[1]);
    dump(dir + "/" + stem + "_valid1.u8", f2c.get_validity_pyr()[1]);
    dump(dir + "/" + stem + "_agree0.i32", counts.agree);
    dump(dir + "/" + stem + "_seen0.i32", counts.seen);
    dump(dir + "/" + stem + "_fused_map.f32", map);
    dump(dir + "/" + stem + "_fused_valid.u8", valid);
    const std::vector<unsigned long long> dropped(1, f2c.get_inconsistent(0));
    dump(dir + "/" + stem + "_dropped0.u64", dropped);
    return rc;
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
    rslfx::Depth1DParameters params;
    int rc = 0;

    // ---- the setter's refusals ----------------------------------------------------------------------------------------------
    F2c off(ctx, epis.data(), rslfx::InputType::F32, V, S, U, 0, -2.0f, 2.0f, D, 1.0f, params);
    if (!refuses([&] { off.set_consistency_gate(2); }))   // before keep_on_device
        rc |= 0x100;
    off.keep_on_device(false);
    if (!refuses([&] { off.set_consistency_gate(-1); }) || !refuses([&] { off.set_consistency_gate(2, std::nanf("")); }) ||
        !refuses([&] { off.set_consistency_gate(2, INFINITY); }))
        rc |= 0x200;
    if (off.get_consistency_min_agree() != 0)   // a refused call sets nothing
        rc |= 0x400;
    if (!refuses([&] { (void)off.get_inconsistent(0); }))   // before run()
        rc |= 0x800;
    off.set_consistency_gate(2, 0.5f, 1);
    off.set_consistency_gate(0);   // off again: the run below is the ungated one
    off.run();
    if (off.get_inconsistent(0) != 0 || off.get_inconsistent(1) != 0 || !refuses([&] { (void)off.get_gate_counts(0); }))
        rc |= 0x1000;
    F2c plain(ctx, epis.data(), rslfx::InputType::F32, V, S, U, 0, -2.0f, 2.0f, D, 1.0f, params);
    plain.keep_on_device(false);
    plain.run();
    std::vector<float> map_off, map_plain;
    std::vector<uint8_t> valid_off, valid_plain;
    off.get_results(map_off, valid_off);
    plain.get_results(map_plain, valid_plain);
    if (!same_bytes(map_off, map_plain) || !same_bytes(valid_off, valid_plain) || !same_bytes(off.get_validity_pyr()[0], plain.get_validity_pyr()[0]))
        rc |= 0x2000;
    dump(dir + "/off_valid0.u8", off.get_validity_pyr()[0]);
    dump(dir + "/off_fused_map.f32", map_off);
    F2c on_multi(multi, epis.data(), rslfx::InputType::F32, V, S, U, 0, -2.0f, 2.0f, D, 1.0f, params);
    if (!refuses([&] { on_multi.set_consistency_gate(2); }))   // one device only
        rc |= 0x4000;

    // ---- gated runs ---------------------------------------------------------------------------------------------------------
    rc |= gated_run(dir, "gate_default", ctx, epis.data(), V, S, U, D, 2, -1.f, 0, off.get_depths_pyr()[0]);
    rc |= gated_run(dir, "gate_picked", ctx, epis.data(), V, S, U, D, 3, 0.3f, 2, off.get_depths_pyr()[0]);
    return rc;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    try {
        const int rc = run(dir);
        std::printf("host f2c consistency: %s (0x%x)\n", rc ? "FAILED" : "ok", rc);
        return rc ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 3;
    }
}
