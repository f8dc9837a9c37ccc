// FineToCoarse of include/rslf_hip.hpp with keep_on_device, used the way the reference's flagship program uses its class
// (RSLightFields/tests/test_fine_to_coarse.cpp:59-75): construct, run, get_results, get_coloured_depth_maps,
// get_coloured_epi_pyr, get_coloured_depth_pyr -- for one float channel and for three uchar channels.  Built with
// g++ -std=c++11 against librslf_hip.so.  Writes the pictures and the planes they were rendered from to <out_dir>/ for the
// pytest side (tests/test_gpu_cpp_f2c_keep.py), which rebuilds every picture with tests/render_ref.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

template <typename T>
static void dump_pyr(const std::string& path, const std::vector<std::vector<T> >& pyr)   // the levels one after the other
{
    std::vector<T> flat;
    for (size_t l = 0; l < pyr.size(); l++)
        flat.insert(flat.end(), pyr[l].begin(), pyr[l].end());
    dump(path, flat);
}

static unsigned g_state = 77u;
static unsigned next16()
{
    g_state = g_state * 1664525u + 1013904223u;
    return (g_state >> 8) & 0xffffu;
}

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

// The same texture in every view, shifted by one column per view on the lower half; a fifth of it in shadow.  T = float:
// levels 3 .. 203; T = uint8_t: 0 .. 255.
template <typename T, int C>
static void make_field(int V, int S, int U, std::vector<std::vector<T> >* epis, std::vector<const void*>* ptrs, std::vector<T>* flat)
{
    epis->assign(V, std::vector<T>());
    ptrs->assign(V, nullptr);
    for (int v = 0; v < V; v++) {
        (*epis)[v].resize((size_t)S * U * C);
        std::vector<float> tex((size_t)(U + 2 * S) * C);
        for (size_t i = 0; i < tex.size(); i += C) {
            const bool dark = next16() % 5 == 0;
            for (int c = 0; c < C; c++) {
                tex[i + c] = 3.0f + 200.0f * (float)next16() / 65535.0f;
                if (dark)
                    tex[i + c] *= 0.04f;
            }
        }
        for (int s = 0; s < S; s++)
            for (int u = 0; u < U; u++)
                for (int c = 0; c < C; c++)
                    (*epis)[v][((size_t)s * U + u) * C + c] = (T)tex[(size_t)(u + S + ((v >= V / 2) ? (s - S / 2) : 0)) * C + c];
        (*ptrs)[v] = (*epis)[v].data();
        flat->insert(flat->end(), (*epis)[v].begin(), (*epis)[v].end());
    }
}

template <typename T, int C>
static int run_case(rslfx::Context& ctx, rslfx::MultiContext& multi, const std::string& dir, const std::string& tag, const uint8_t* lut)
{
    const int V = 44, S = 5, U = 64, D = 9;
    const rslfx::InputType type = sizeof(T) == 1 ? rslfx::InputType::U8 : rslfx::InputType::F32;
    std::vector<std::vector<T> > epis;
    std::vector<const void*> ptrs;
    std::vector<T> flat;
    make_field<T, C>(V, S, U, &epis, &ptrs, &flat);
    dump(dir + "/" + tag + "_input.raw", flat);
    rslfx::Depth1DParameters params;
    if (!params.par_cut_shadows)
        return 1;
    dump(dir + "/shadow_level.f32", std::vector<float>(1, params.par_shadow_level));

    // the setters' refusals: a validity rule without keep_on_device, a kept run on several devices
    rslfx::FineToCoarse<C> f2c(ctx, ptrs.data(), type, V, S, U, 0, -1.0f, 1.0f, D, -1, params);
    if (!refuses([&] { f2c.set_validity_rule(RSLF_F2C_VALID_REFERENCE); }))
        return 2;
    rslfx::FineToCoarse<C> on_multi(multi, ptrs.data(), type, V, S, U, 0, -1.0f, 1.0f, D, -1, params);
    if (!refuses([&] { on_multi.keep_on_device(); }))
        return 4;
    if (!refuses([&] { f2c.get_coloured_epi_pyr(-1, lut); }))   // before keep_on_device + run() there is nothing on the device
        return 8;

    // the reference's sequence (test_fine_to_coarse.cpp:59-75)
    f2c.keep_on_device();
    if (!refuses([&] { f2c.set_validity_rule(7); }))
        return 16;
    f2c.set_validity_rule(RSLF_F2C_VALID_COMPAT);
    f2c.run();
    std::vector<float> map;
    std::vector<uint8_t> valid;
    f2c.get_results(map, valid);
    const Picture maps = f2c.get_coloured_depth_maps(lut);
    const std::vector<Picture> epi_pyr = f2c.get_coloured_epi_pyr(-1, lut);
    const std::vector<Picture> depth_pyr = f2c.get_coloured_depth_pyr(-1, lut);
    if ((int)epi_pyr.size() != f2c.pyramid_depth() || (int)depth_pyr.size() != f2c.pyramid_depth() ||
        (int)f2c.pyramid_dims().size() != f2c.pyramid_depth() || f2c.pyramid_depth() != 3)
        return 32;
    dump(dir + "/" + tag + "_map.f32", map);
    dump(dir + "/" + tag + "_valid.u8", valid);
    dump(dir + "/" + tag + "_maps.u8", maps);
    dump_pyr(dir + "/" + tag + "_epi_pyr.u8", epi_pyr);
    dump_pyr(dir + "/" + tag + "_depth_pyr.u8", depth_pyr);
    dump_pyr(dir + "/" + tag + "_depths.f32", f2c.get_depths_pyr());
    dump_pyr(dir + "/" + tag + "_validity.u8", f2c.get_validity_pyr());
    dump_pyr(dir + "/" + tag + "_disp_conf.f32", f2c.get_disp_confidence_pyr());
    dump_pyr(dir + "/" + tag + "_epi_pyr_5_unsaturated.u8", f2c.get_coloured_epi_pyr(5, lut, false));
    if (!f2c.get_line_confidence_pyr().empty())   // no line mode was set
        return 64;
    if (f2c.get_depths_pyr().size() != 3 || f2c.get_depths_pyr()[1].size() != (size_t)S * 22 * 32)
        return 128;
    if (!refuses([&] { f2c.get_coloured_epi_pyr(V - 1, lut); }))   // round(43 * 22 / 44) = 22 is past level 1's last row
        return 256;

    // an object without keep_on_device gives the same results, and the same picture through its second upload
    rslfx::FineToCoarse<C> plain(ctx, ptrs.data(), type, V, S, U, 0, -1.0f, 1.0f, D, -1, params);
    plain.run();
    std::vector<float> map_p;
    std::vector<uint8_t> valid_p;
    plain.get_results(map_p, valid_p);
    if (map_p.size() != map.size() || std::memcmp(map_p.data(), map.data(), map.size() * sizeof(float)) != 0 || valid_p != valid) {
        std::fprintf(stderr, "%s: get_results of the kept run differs from the plain run's\n", tag.c_str());
        return 512;
    }
    if (plain.get_coloured_depth_maps(lut) != maps || plain.stats.pixels_scanned != f2c.stats.pixels_scanned) {
        std::fprintf(stderr, "%s: the kept run's picture or stats differ from the plain run's\n", tag.c_str());
        return 1024;
    }
    // a second run() on the same object replaces the first
    f2c.run();
    if (f2c.get_coloured_depth_maps(lut) != maps)
        return 2048;
    return 0;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    try {
        std::vector<uint8_t> lut(256 * 3);
        for (size_t i = 0; i < lut.size(); i++)
            lut[i] = (uint8_t)(1u + (next16() % 255u));   // no black entry: black is the masks' and the shadow cut's
        dump(dir + "/lut.u8", lut);
        rslfx::Context ctx(0);
        rslfx::MultiContext multi(std::vector<int>(1, 0));
        int rc = run_case<float, 1>(ctx, multi, dir, "c1", lut.data());
        rc |= run_case<uint8_t, 3>(ctx, multi, dir, "c3", lut.data()) << 12;
        std::printf("host f2c keep: %s (0x%x)\n", rc ? "FAILED" : "ok", rc);
        return rc ? 1 : 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 3;
    }
}
