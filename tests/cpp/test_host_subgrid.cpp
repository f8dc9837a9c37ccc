// rslfx::Depth1DComputer_pile::set_subgrid (include/rslf_hip.hpp): the sub-grid pile step through the C++11 host wrapper.
// Built with g++ -std=c++11 against librslf_hip.so.  Reads <dir>/volume.f32, a [7][9][96] float field that
// tests/test_gpu_cpp_subgrid.py wrote, runs the pile computer on it with the mode off and on and compares the members with
// what the C-ABI host entry (rslf_depth1d_pile_run_host_sub) gives for the same volume; the planes are also written out for
// the pytest side, which compares them with the Python class's.  An object built on a MultiContext must refuse the mode with
// std::invalid_argument, and still run with it off.
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

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b)
{
    if (a.size() != b.size())
        return false;
    for (size_t k = 0; k < a.size(); k++)
        if (a[k] != b[k])   // (no NaN in these planes)
            return false;
    return true;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    const int V = 7, S = 9, U = 96, D = 9;
    typedef rslfx::Depth1DComputer_pile<1> Pile;
    try {
        std::vector<float> field((size_t)V * S * U);
        FILE* f = std::fopen((dir + "/volume.f32").c_str(), "rb");
        if (!f || std::fread(field.data(), sizeof(float), field.size(), f) != field.size()) {
            std::perror("volume.f32");
            return 2;
        }
        std::fclose(f);
        std::vector<const void*> ptrs(V);
        for (int v = 0; v < V; v++)
            ptrs[v] = field.data() + (size_t)v * S * U;

        rslfx::Context ctx(0);
        Pile pile(ctx, ptrs.data(), false, V, S, U, 0, -1.0f, 1.0f, D, -1, 1.0f);
        if (pile.get_subgrid())   // default off
            return 1;
        pile.run();
        const std::vector<float> grid_depth = pile.m_best_depth_v_u, grid_score = pile.m_score_v_u, grid_Cd = pile.m_disp_confidence_v_u;
        const std::vector<int32_t> grid_idx = pile.m_depth_idx_v_u;
        pile.set_subgrid(true);
        pile.run();
        if (pile.m_depth_idx_v_u != grid_idx || !same_bits(pile.m_score_v_u, grid_score) || !same_bits(pile.m_disp_confidence_v_u, grid_Cd)) {
            std::printf("host subgrid: FAILED: the mode changed idx, score or C_d\n");
            return 1;
        }
        if (same_bits(pile.m_best_depth_v_u, grid_depth)) {
            std::printf("host subgrid: FAILED: the mode changed nothing\n");
            return 1;
        }
        dump(dir + "/depth_grid.f32", grid_depth);
        dump(dir + "/depth_sub.f32", pile.m_best_depth_v_u);
        dump(dir + "/idx.i32", pile.m_depth_idx_v_u);
        dump(dir + "/mask.u8", pile.m_edge_confidence_mask_v_u);

        // the C entry on a second volume of the same field: the members, bit for bit, with the mode on and off
        {
            rslfx::Context other(0);
            rslf_volume* vol = nullptr;
            rslfx::check(rslf_volume_create(other.get(), V, S, U, 1, &vol), "rslf_volume_create");
            float used = 0.0f;
            int rc = rslf_volume_upload_epis_f32(vol, (const float* const*)ptrs.data(), 0, 1.0f, &used);
            const size_t n = (size_t)V * U;
            rslf_params p;
            rslf_default_params(&p);   // (the computer above was built with the defaults)
            for (int sub = 1; sub >= 0 && rc == RSLF_OK; sub--) {
                std::vector<float> Ce(n, 5.0f), Cd(n, 5.0f), depth(n, 5.0f), rbar(n, 5.0f), score(n, 5.0f);
                std::vector<uint8_t> mask(n, 5);
                std::vector<int32_t> idx(n, 5);
                rc = rslf_depth1d_pile_run_host_sub(other.get(), vol, -1.0f, 1.0f, D, -1, &p, Ce.data(), mask.data(), Cd.data(), depth.data(),
                                                    rbar.data(), idx.data(), score.data(), nullptr, nullptr, sub);
                if (rc != RSLF_OK)
                    break;
                const bool equal = same_bits(depth, sub ? pile.m_best_depth_v_u : grid_depth) && idx == grid_idx && same_bits(score, grid_score) &&
                                   mask == pile.m_edge_confidence_mask_v_u && same_bits(Cd, grid_Cd) && same_bits(rbar, pile.m_rbar_v_u);
                if (!equal) {
                    std::printf("host subgrid: FAILED: set_subgrid(%d) and rslf_depth1d_pile_run_host_sub differ\n", sub);
                    rslf_volume_destroy(vol);
                    return 1;
                }
            }
            rslf_volume_destroy(vol);
            rslfx::check(rc, "rslf_depth1d_pile_run_host_sub");
        }
        // back off: the grid planes again
        pile.set_subgrid(false);
        pile.run();
        if (!same_bits(pile.m_best_depth_v_u, grid_depth))
            return 1;

        // the MultiContext form: the mode is refused, naming the reason; with it off the object runs as before
        rslfx::MultiContext multi(std::vector<int>(2, 0));
        Pile shared(multi, ptrs.data(), false, V, S, U, 0, -1.0f, 1.0f, D, -1, 1.0f);
        bool threw = false;
        try {
            shared.set_subgrid(true);
        } catch (const std::invalid_argument& e) {
            threw = std::string(e.what()).find("MultiContext") != std::string::npos;
        }
        shared.set_subgrid(false);
        shared.run();
        if (shared.get_subgrid() || !same_bits(shared.m_best_depth_v_u, grid_depth))
            return 1;
        std::printf("host subgrid: %s\n", threw ? "ok" : "FAILED: the MultiContext form did not throw std::invalid_argument");
        return threw ? 0 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 3;
    }
}
