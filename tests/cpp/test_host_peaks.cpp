// rslfx::Depth1DComputer_pile::get_peaks (include/rslf_hip.hpp): the score-row peaks through the C++11 host wrapper.
// Built with g++ -std=c++11 against librslf_hip.so.  Reads <dir>/volume.f32, a [3][17][150][3] float field in [0, 1) that
// tests/test_gpu_cpp_peaks.py wrote, runs the pile computer on it and compares the getter's five planes -- of every
// scanline, and of a window -- with what the C-ABI host form (rslf_depth_epi_peaks_host) gives for the same volume, mask and
// range; the planes are also written out for the pytest side, which compares them with the Python getter's.  The object
// built on a MultiContext must refuse with std::invalid_argument.
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

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    const int V = 3, S = 17, U = 150, D = 24, C = 3;
    typedef rslfx::Depth1DComputer_pile<3> Pile;
    try {
        std::vector<float> field((size_t)V * S * U * C);
        FILE* f = std::fopen((dir + "/volume.f32").c_str(), "rb");
        if (!f || std::fread(field.data(), sizeof(float), field.size(), f) != field.size()) {
            std::perror("volume.f32");
            return 2;
        }
        std::fclose(f);
        std::vector<const void*> ptrs(V);
        for (int v = 0; v < V; v++)
            ptrs[v] = field.data() + (size_t)v * S * U * C;

        rslfx::Context ctx(0);
        Pile pile(ctx, ptrs.data(), false, V, S, U, 0, -2.0f, 5.0f, D, -1, 1.0f);
        bool refused = false;
        try {
            pile.get_peaks();   // before run() there is nothing to show
        } catch (const rslfx::Error& e) {
            refused = e.status == RSLF_ERR_INVALID_ARG;
        }
        if (!refused)
            return 1;
        pile.run();
        const Pile::Peaks all = pile.get_peaks();
        const size_t n = (size_t)V * U;
        if (all.idx.size() != n || all.score.size() != n || all.disp.size() != n || all.runner_idx.size() != n || all.runner_score.size() != n)
            return 1;
        if (all.idx != pile.m_depth_idx_v_u)   // the winner is the scan's arg max, -1 where no disparity was assigned
            return 1;
        const Pile::Peaks row1 = pile.get_peaks(1, 1);
        for (int u = 0; u < U; u++)
            if (row1.idx[u] != all.idx[U + u] || row1.disp[u] != all.disp[U + u] || row1.runner_idx[u] != all.runner_idx[U + u])
                return 1;
        dump(dir + "/idx.i32", all.idx);
        dump(dir + "/score.f32", all.score);
        dump(dir + "/disp.f32", all.disp);
        dump(dir + "/runner_idx.i32", all.runner_idx);
        dump(dir + "/runner_score.f32", all.runner_score);
        dump(dir + "/mask.u8", pile.m_edge_confidence_mask_v_u);
        refused = false;
        try {
            pile.get_peaks(2, 2);   // not a window of three scanlines
        } catch (const rslfx::Error& e) {
            refused = e.status == RSLF_ERR_INVALID_ARG;
        }
        if (!refused)
            return 1;

        // the C-ABI host form on a second volume of the same field: the getter's planes, bit for bit
        {
            rslfx::Context other(0);
            rslf_volume* vol = nullptr;
            rslfx::check(rslf_volume_create(other.get(), V, S, U, C, &vol), "rslf_volume_create");
            float used = 0.0f;
            int rc = rslf_volume_upload_epis_f32(vol, (const float* const*)ptrs.data(), 0, 1.0f, &used);
            std::vector<int32_t> idx(n, 5), runner(n, 5);
            std::vector<float> score(n, 5.0f), disp(n, 5.0f), rscore(n, 5.0f);
            const rslf_peaks planes = {idx.data(), score.data(), disp.data(), runner.data(), rscore.data()};
            rslf_params p;
            rslf_default_params(&p);   // (the computer above was built with the defaults)
            if (rc == RSLF_OK)
                rc = rslf_depth_epi_peaks_host(other.get(), vol, nullptr, nullptr, -2.0f, 5.0f, D, pile.get_s_hat(), &p,
                                               pile.m_edge_confidence_mask_v_u.data(), 0, V, &planes, nullptr);
            rslf_volume_destroy(vol);
            rslfx::check(rc, "rslf_depth_epi_peaks_host");
            bool equal = idx == all.idx && runner == all.runner_idx;
            for (size_t k = 0; k < n && equal; k++)
                equal = score[k] == all.score[k] && disp[k] == all.disp[k] && rscore[k] == all.runner_score[k];
            if (!equal) {
                std::printf("host peaks: FAILED: the getter and rslf_depth_epi_peaks_host differ\n");
                return 1;
            }
        }

        // the MultiContext form keeps no volume on a device: it throws, naming the reason
        rslfx::MultiContext multi(std::vector<int>(2, 0));
        Pile shared(multi, ptrs.data(), false, V, S, U, 0, -2.0f, 5.0f, D, -1, 1.0f);
        shared.run();
        if (shared.m_depth_idx_v_u != pile.m_depth_idx_v_u)
            return 1;
        bool threw = false;
        try {
            shared.get_peaks();
        } catch (const std::invalid_argument& e) {
            threw = std::string(e.what()).find("MultiContext") != std::string::npos;
        }
        std::printf("host peaks: %s\n", threw ? "ok" : "FAILED: the MultiContext form did not throw std::invalid_argument");
        return threw ? 0 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 3;
    }
}
