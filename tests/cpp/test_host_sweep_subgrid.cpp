// rslfx::Depth2DComputer::set_subgrid and rslfx::FineToCoarse::set_subgrid (include/rslf_hip.hpp): the sub-grid 2-D sweep and
// pyramid through the C++11 host wrapper.  Built with g++ -std=c++11 against librslf_hip.so.  Reads <dir>/sweep.f32, the
// [6][5][80] planted field, and <dir>/pyramid.f32, a [44][5][64] field, both written by tests/test_gpu_cpp_sweep_subgrid.py; runs
// both classes with the mode off and on and writes the planes out for the pytest side, which compares them with the Python
// objects'.  Objects built on a MultiContext must refuse the mode with std::invalid_argument.
#include <cstdio>
#include <cstdlib>
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

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b)
{
    if (a.size() != b.size())
        return false;
    for (size_t k = 0; k < a.size(); k++)
        if (a[k] != b[k])   // (no NaN in these planes)
            return false;
    return true;
}

template <typename Obj>
static bool refuses(Obj& o)
{
    try {
        o.set_subgrid(true);
    } catch (const std::invalid_argument& e) {
        o.set_subgrid(false);   // off is always accepted
        return std::string(e.what()).find("MultiContext") != std::string::npos && !o.get_subgrid();
    }
    return false;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    try {
        rslfx::Context ctx(0);
        rslfx::MultiContext multi(std::vector<int>(2, 0));
        {   // the sweep
            const int V = 6, S = 5, U = 80, D = 9;
            const std::vector<float> field = load(dir + "/sweep.f32", (size_t)V * S * U);
            std::vector<const void*> ptrs(V);
            for (int v = 0; v < V; v++)
                ptrs[v] = field.data() + (size_t)v * S * U;
            rslfx::Depth2DComputer<1> comp(ctx, ptrs.data(), false, V, S, U, 0, -2.0f, 2.0f, D, 1.0f);
            if (comp.get_subgrid())   // default off
                return 1;
            comp.run();
            const std::vector<float> grid = comp.get_depths_s_v_u();
            dump(dir + "/sweep_depth_grid.f32", grid);
            comp.set_subgrid(true);
            comp.run();
            if (same_bits(comp.get_depths_s_v_u(), grid)) {
                std::printf("host sweep subgrid: FAILED: the mode changed nothing\n");
                return 1;
            }
            dump(dir + "/sweep_depth_sub.f32", comp.get_depths_s_v_u());
            dump(dir + "/sweep_Ce.f32", comp.m_edge_confidence_s_v_u);
            dump(dir + "/sweep_mask.u8", comp.m_edge_confidence_mask_s_v_u);
            dump(dir + "/sweep_Cd.f32", comp.m_disp_confidence_s_v_u);
            dump(dir + "/sweep_rbar.f32", comp.m_rbar_s_v_u);
            comp.set_subgrid(false);   // back off: the grid planes again
            comp.run();
            if (!same_bits(comp.get_depths_s_v_u(), grid))
                return 1;
            rslfx::Depth2DComputer<1> shared(multi, ptrs.data(), false, V, S, U, 0, -2.0f, 2.0f, D, 1.0f);
            if (!refuses(shared)) {
                std::printf("host sweep subgrid: FAILED: Depth2DComputer on a MultiContext did not throw std::invalid_argument\n");
                return 1;
            }
        }
        {   // the pyramid: the levels_out run and the kept run
            const int V = 44, S = 5, U = 64, D = 9;
            const std::vector<float> field = load(dir + "/pyramid.f32", (size_t)V * S * U);
            std::vector<const void*> ptrs(V);
            for (int v = 0; v < V; v++)
                ptrs[v] = field.data() + (size_t)v * S * U;
            std::vector<float> map, kept_map;
            std::vector<uint8_t> valid, kept_valid;
            rslfx::FineToCoarse<1> f2c(ctx, ptrs.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
            if (f2c.get_subgrid())
                return 1;
            f2c.set_subgrid(true);
            f2c.run();
            f2c.get_results(map, valid);
            dump(dir + "/f2c_map.f32", map);
            dump(dir + "/f2c_valid.u8", valid);
            for (size_t l = 0; l < f2c.get_depths_pyr().size(); l++)
                dump(dir + "/f2c_depth_" + std::to_string(l) + ".f32", f2c.get_depths_pyr()[l]);
            rslfx::FineToCoarse<1> kept(ctx, ptrs.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
            kept.keep_on_device();
            kept.set_subgrid(true);
            kept.run();
            kept.get_results(kept_map, kept_valid);
            if (!same_bits(kept_map, map) || kept_valid != valid || kept.pyramid_depth() != f2c.pyramid_depth()) {
                std::printf("host sweep subgrid: FAILED: the kept run and the levels run differ\n");
                return 1;
            }
            rslfx::FineToCoarse<1> plain(ctx, ptrs.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
            plain.run();
            std::vector<float> grid_map;
            std::vector<uint8_t> grid_valid;
            plain.get_results(grid_map, grid_valid);
            dump(dir + "/f2c_map_grid.f32", grid_map);
            if (same_bits(grid_map, map)) {
                std::printf("host sweep subgrid: FAILED: the mode changed nothing in the pyramid\n");
                return 1;
            }
            rslfx::FineToCoarse<1> shared(multi, ptrs.data(), false, V, S, U, 0, -1.0f, 1.0f, D);
            if (!refuses(shared)) {
                std::printf("host sweep subgrid: FAILED: FineToCoarse on a MultiContext did not throw std::invalid_argument\n");
                return 1;
            }
        }
        std::printf("host sweep subgrid: ok\n");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 3;
    }
}
