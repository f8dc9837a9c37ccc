// The picture getters of include/rslf_hip.hpp, used the way the reference's demos use theirs
// (RSLightFields/tests/test_depth_computation_pile.cpp, test_depth_computation_2d.cpp:77, test_fine_to_coarse.cpp):
//     depth_computer.run();  ... = depth_computer.get_coloured_epi(...);  ... = depth_computer.get_disparity_map(...);
// Built with g++ -std=c++11 against librslf_hip.so; no OpenCV here, so pictures are byte vectors and the colour map is
// a table.  Writes every picture, and the result planes it was rendered from, to <out_dir>/ for the pytest side
// (tests/test_gpu_cpp_getters.py), which rebuilds the pictures with tests/render_ref.py and compares bytes.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rslf_hip.hpp"

typedef std::vector<uint8_t> Picture;

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

static unsigned g_state = 2024u;
static unsigned next16()
{
    g_state = g_state * 1664525u + 1013904223u;
    return (g_state >> 8) & 0xffffu;
}

// true when `call` throws rslfx::Error with RSLF_ERR_INVALID_ARG
template <typename F>
static bool refuses(F call)
{
    try {
        call();
    } catch (const rslfx::Error& e) {
        return e.status == RSLF_ERR_INVALID_ARG;
    }
    return false;
}

static int run_pile(rslfx::Context& ctx, const std::string& dir, const uint8_t* lut)
{
    const int V = 7, S = 13, U = 150, D = 20;
    std::vector<std::vector<float> > epis(V);
    std::vector<const void*> ptrs(V);
    for (int v = 0; v < V; v++) {
        epis[v].resize((size_t)S * U);
        for (size_t i = 0; i < epis[v].size(); i++)
            epis[v][i] = 3.0f + 250.0f * (float)next16() / 65535.0f;
        ptrs[v] = epis[v].data();
    }
    rslfx::Depth1DComputer_pile<1> pile(ctx, ptrs.data(), false, V, S, U, 0, -1.5f, 2.0f, D);
    if (!refuses([&] { pile.get_disparity_map(lut); }))   // before run() there is nothing to show
        return 1;
    pile.run();
    dump(dir + "/pile_depth.f32", pile.m_best_depth_v_u);
    dump(dir + "/pile_mask.u8", pile.m_edge_confidence_mask_v_u);
    dump(dir + "/pile_s_hat.i32", std::vector<int>(1, pile.get_s_hat()));
    dump(dir + "/pile_epi_default.u8", pile.get_coloured_epi(-1, lut));
    dump(dir + "/pile_epi_5.u8", pile.get_coloured_epi(5, lut));
    dump(dir + "/pile_map.u8", pile.get_disparity_map(lut));
    if (pile.get_disparity_map(lut) != pile.get_disparity_map(ctx, lut))   // the second call allocates nothing and gives the same bytes
        return 1;
    return refuses([&] { pile.get_coloured_epi(V, lut); }) ? 0 : 1;
}

static int run_sweeps(rslfx::Context& ctx, const std::string& dir, const uint8_t* lut)
{
    const int V = 44, S = 5, U = 64, D = 9;
    std::vector<std::vector<float> > epis(V);
    std::vector<const void*> ptrs(V);
    std::vector<float> flat;
    for (int v = 0; v < V; v++) {
        epis[v].resize((size_t)S * U);
        // the same texture in every view, shifted by one column per view on the lower half; some of it in shadow
        std::vector<float> tex(U + 2 * S);
        for (size_t i = 0; i < tex.size(); i++) {
            tex[i] = 3.0f + 200.0f * (float)next16() / 65535.0f;
            if (next16() % 5 == 0)
                tex[i] *= 0.04f;
        }
        for (int s = 0; s < S; s++)
            for (int u = 0; u < U; u++)
                epis[v][(size_t)s * U + u] = tex[u + S + ((v >= V / 2) ? (s - S / 2) : 0)];
        ptrs[v] = epis[v].data();
        flat.insert(flat.end(), epis[v].begin(), epis[v].end());
    }
    dump(dir + "/sweep_input.f32", flat);

    rslfx::Depth2DComputer<1> d2(ctx, ptrs.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
    d2.run();
    dump(dir + "/d2_depth.f32", d2.get_depths_s_v_u());
    dump(dir + "/d2_mask.u8", d2.m_edge_confidence_mask_s_v_u);
    dump(dir + "/d2_epi_default.u8", d2.get_coloured_epi(-1, lut));
    dump(dir + "/d2_epi_43.u8", d2.get_coloured_epi(43, lut));
    dump(dir + "/d2_map_default.u8", d2.get_disparity_map(-1, lut));
    dump(dir + "/d2_map_0.u8", d2.get_disparity_map(0, lut));
    const Picture maps = d2.get_disparity_maps(lut), slices = d2.get_coloured_epis(lut);
    dump(dir + "/d2_maps.u8", maps);
    dump(dir + "/d2_epis.u8", slices);
    if (!refuses([&] { d2.get_disparity_map(S, lut); }) || !refuses([&] { d2.get_coloured_epi(V, lut); }))
        return 4;

    // with par_use_disp_confidence_score the getters paint under C_d > threshold
    rslfx::Depth1DParameters by_score;
    by_score.par_use_disp_confidence_score = true;
    rslfx::Depth2DComputer<1> d2s(ctx, ptrs.data(), false, V, S, U, 0, -1.0f, 1.0f, D, -1, by_score);
    d2s.run();
    dump(dir + "/d2s_depth.f32", d2s.get_depths_s_v_u());
    dump(dir + "/d2s_conf.f32", d2s.m_disp_confidence_s_v_u);
    dump(dir + "/d2s_threshold.f32", std::vector<float>(1, by_score.par_disp_score_threshold));
    dump(dir + "/d2s_maps.u8", d2s.get_disparity_maps(lut));

    // an object built on a MultiContext has no context of its own: the getters take the one to render on
    rslfx::MultiContext multi(std::vector<int>(1, 0));
    rslfx::Depth2DComputer<1> d2m(multi, ptrs.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
    d2m.run();
    bool threw = false;
    try {
        d2m.get_disparity_maps(lut);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw || d2m.get_disparity_maps(ctx, lut) != maps || d2m.get_coloured_epis(ctx, lut) != slices ||
        d2m.get_disparity_map(ctx, 0, lut) != d2.get_disparity_map(0, lut) || d2m.get_coloured_epi(ctx, -1, lut) != d2.get_coloured_epi(-1, lut)) {
        std::fprintf(stderr, "the getters of the MultiContext object differ\n");
        return 8;
    }

    rslfx::Depth1DParameters params;
    dump(dir + "/shadow_level.f32", std::vector<float>(1, params.par_shadow_level));
    if (!params.par_cut_shadows)
        return 16;
    rslfx::FineToCoarse<1> f2c(ctx, ptrs.data(), false, V, S, U, 0, -1.0f, 1.0f, D, -1, params);
    f2c.run();
    std::vector<float> map;
    std::vector<uint8_t> valid;
    f2c.get_results(map, valid);
    dump(dir + "/f2c_map.f32", map);
    dump(dir + "/f2c_valid.u8", valid);
    const Picture cut = f2c.get_coloured_depth_maps(lut);
    dump(dir + "/f2c_maps_cut.u8", cut);
    params.par_cut_shadows = false;
    rslfx::FineToCoarse<1> plain(ctx, ptrs.data(), false, V, S, U, 0, -1.0f, 1.0f, D, -1, params);
    plain.run();
    std::vector<float> map_p;
    std::vector<uint8_t> valid_p;
    plain.get_results(map_p, valid_p);
    dump(dir + "/f2c_plain_map.f32", map_p);
    dump(dir + "/f2c_plain_valid.u8", valid_p);
    dump(dir + "/f2c_maps_plain.u8", plain.get_coloured_depth_maps(lut, true));
    rslfx::FineToCoarse<1> f2cm(multi, ptrs.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
    f2cm.run();
    if (f2cm.get_coloured_depth_maps(ctx, lut) != cut) {
        std::fprintf(stderr, "get_coloured_depth_maps of the MultiContext object differs\n");
        return 32;
    }
    // one view: (int)std::round(1 / 2.0) is 1, the reference reads past its last plane
    rslfx::FineToCoarse<1> one(ctx, ptrs.data(), false, V, 1, U, 0, -1.0f, 1.0f, D);
    return refuses([&] { one.get_coloured_depth_maps(lut); }) ? 0 : 64;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    try {
        std::vector<uint8_t> lut(256 * 3);
        for (size_t i = 0; i < lut.size(); i++)
            lut[i] = (uint8_t)(next16() & 0xffu);
        dump(dir + "/lut.u8", lut);
        rslfx::Context ctx(0);
        int rc = run_pile(ctx, dir, lut.data());
        rc |= run_sweeps(ctx, dir, lut.data());
        std::printf("host getters: %s (0x%x)\n", rc ? "FAILED" : "ok", rc);
        return rc;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 3;
    }
}
