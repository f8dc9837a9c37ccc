// The sweep gate through the C++11 host wrapper (include/rslf_hip.hpp): rslfx::Depth2DComputer::set_propagation_ratio /
// get_propagation_ratio / get_withheld_sources, and the same on a kept rslfx::FineToCoarse with get_withheld_sources(level).
// Built with g++ -std=c++11 against librslf_hip.so.  Reads <dir>/level0.f32 -- the normalised level 0 of case A, [44][5][64] --
// and <dir>/input.f32, the raw field; runs the classes at the ratio 0.7 and writes planes and counts out for the pytest side
// (tests/test_gpu_cpp_sweep_gate.py), which holds them to the numpy yardstick.  Here: the setters' refusals, r = 1 and the
// ratio switched off again give the ungated planes, and every plane of the classes equals what the C entries give.
#include <cstdio>
#include <cstdlib>
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
static bool same(const std::vector<T>& a, const std::vector<T>& b)
{
    if (a.size() != b.size())
        return false;
    for (size_t k = 0; k < a.size(); k++)
        if (a[k] != b[k])   // (no NaN in these planes)
            return false;
    return true;
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
    const int V = 44, S = 5, U = 64, D = 9;
    const float ratio = 0.7f;
    const size_t n = (size_t)S * V * U;
    const std::vector<float> level0 = load(dir + "/level0.f32", n), raw = load(dir + "/input.f32", n);
    std::vector<const void*> p0(V), pr(V);
    for (int v = 0; v < V; v++) {
        p0[v] = level0.data() + (size_t)v * S * U;
        pr[v] = raw.data() + (size_t)v * S * U;
    }
    rslfx::Context ctx(0);
    rslfx::MultiContext multi(std::vector<int>(1, 0));
    int rc = 0;

    // ---- Depth2DComputer --------------------------------------------------------------------------------------------------
    Sweep comp(ctx, p0.data(), false, V, S, U, 0, -1.0f, 1.0f, D, 1.0f);
    if (!refuses([&] { comp.set_propagation_ratio(1.5f); }) || !refuses([&] { comp.set_propagation_ratio(-0.5f); }))
        rc |= 1;
    if (!refuses([&] { (void)comp.get_withheld_sources(); }))   // before run()
        rc |= 1;
    comp.set_propagation_ratio(ratio);
    if (comp.get_propagation_ratio() != ratio || !refuses([&] { comp.run(); }))   // the ratio reads the peak planes
        rc |= 2;
    comp.set_peaks(true);
    comp.set_propagation_ratio(0.0f);
    comp.run();
    const std::vector<float> open_depth = comp.get_depths_s_v_u();
    const std::vector<int32_t> open_idx = comp.get_peaks().idx;
    if (comp.get_withheld_sources() != 0)
        rc |= 4;
    comp.set_propagation_ratio(1.0f);   // the gated kernel runs, nothing is withheld
    comp.run();
    if (!same(comp.get_depths_s_v_u(), open_depth) || !same(comp.get_peaks().idx, open_idx) || comp.get_withheld_sources() != 0)
        rc |= 8;
    comp.set_propagation_ratio(ratio);
    comp.run();
    const unsigned long long withheld = comp.get_withheld_sources();
    if (withheld == 0 || same(comp.get_depths_s_v_u(), open_depth))
        rc |= 16;
    dump(dir + "/gate_depth.f32", comp.get_depths_s_v_u());
    dump(dir + "/gate_Cd.f32", comp.m_disp_confidence_s_v_u);
    dump(dir + "/gate_idx.i32", comp.get_peaks().idx);
    dump(dir + "/gate_score.f32", comp.get_peaks().score);
    dump(dir + "/gate_runner_idx.i32", comp.get_peaks().runner_idx);
    dump(dir + "/gate_runner_score.f32", comp.get_peaks().runner_score);
    comp.set_propagation_ratio(0.0f);   // off again: the ungated planes, and 0
    comp.run();
    if (!same(comp.get_depths_s_v_u(), open_depth) || comp.get_withheld_sources() != 0)
        rc |= 32;
    Sweep shared(multi, p0.data(), false, V, S, U, 0, -1.0f, 1.0f, D, 1.0f);
    if (!refuses([&] { shared.set_propagation_ratio(ratio); }) || !refuses([&] { (void)shared.get_withheld_sources(); }))
        rc |= 64;
    shared.set_propagation_ratio(0.0f);   // off is always accepted

    // ---- FineToCoarse, a kept run --------------------------------------------------------------------------------------------
    rslfx::Depth1DParameters params;
    F2c f2c(ctx, pr.data(), rslfx::InputType::F32, V, S, U, 0, -1.0f, 1.0f, D, -1, params);
    if (!refuses([&] { f2c.set_propagation_ratio(ratio); }))   // not a kept run yet
        rc |= 128;
    F2c on_multi(multi, pr.data(), rslfx::InputType::F32, V, S, U, 0, -1.0f, 1.0f, D, -1, params);
    if (!refuses([&] { on_multi.set_propagation_ratio(ratio); }))
        rc |= 256;
    f2c.keep_on_device(false);
    if (!refuses([&] { f2c.set_propagation_ratio(1.5f); }) || !refuses([&] { (void)f2c.get_withheld_sources(0); }))
        rc |= 512;
    f2c.set_propagation_ratio(ratio);
    if (f2c.get_propagation_ratio() != ratio || !refuses([&] { f2c.run(); }))   // needs set_peaks(true)
        rc |= 1024;
    f2c.set_peaks(true);
    f2c.run();
    if (f2c.pyramid_depth() != 3)
        rc |= 2048;
    // the same arguments through the C entry
    const rslf_params p = params.to_c();
    rslf_f2c_run* c_run = nullptr;
    rslf_stats st;
    if (rslf_f2c_run_host_pr(ctx.get(), pr.data(), RSLF_ELEM_F32, V, S, U, 1, 0, -1.0f, 1.0f, D, -1.0f, &p, -1, 1, RSLF_LINE_CONF_OFF,
                             RSLF_F2C_VALID_COMPAT, 0, &c_run, &st, 0, 1, 0.0f, ratio) != RSLF_OK) {
        std::fprintf(stderr, "rslf_f2c_run_host_pr: %s\n", rslf_last_error());
        return rc | 4096;
    }
    if (rslf_f2c_run_propagation_ratio(c_run) != ratio || st.pixels_scanned != f2c.stats.pixels_scanned)
        rc |= 8192;
    std::vector<unsigned long long> counts;
    for (int l = 0; l < f2c.pyramid_depth(); l++) {
        unsigned long long c = 0;
        if (rslf_f2c_run_withheld(c_run, l, &c) != RSLF_OK || c != f2c.get_withheld_sources(l))
            rc |= 16384;
        counts.push_back(f2c.get_withheld_sources(l));
        const size_t nl = (size_t)S * f2c.pyramid_dims()[l].first * f2c.pyramid_dims()[l].second;
        std::vector<float> depth(nl);
        if (rslf_f2c_run_copy(c_run, l, RSLF_F2C_PLANE_DEPTH, depth.data(), 1, nullptr) != RSLF_OK || !same(depth, f2c.get_depths_pyr()[l]))
            rc |= 32768;
    }
    if (!refuses([&] { (void)f2c.get_withheld_sources(3); }))
        rc |= 65536;
    rslf_f2c_run_destroy(c_run);
    std::vector<float> map;
    std::vector<uint8_t> valid;
    f2c.get_results(map, valid);
    dump(dir + "/f2c_fused_map.f32", map);
    dump(dir + "/f2c_depth0.f32", f2c.get_depths_pyr()[0]);
    FILE* f = std::fopen((dir + "/counts.txt").c_str(), "w");
    if (!f)
        return rc | (1 << 17);
    std::fprintf(f, "%llu %llu %llu %llu\n", withheld, counts[0], counts[1], counts[2]);
    std::fclose(f);
    return rc;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    try {
        const int rc = run(dir);
        std::printf("host sweep gate: %s (0x%x)\n", rc ? "FAILED" : "ok", rc);
        return rc ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 3;
    }
}
