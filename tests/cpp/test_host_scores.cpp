// rslfx::Depth1DComputer_pile::get_scores (include/rslf_hip.hpp): the scan's score rows through the C++11 host wrapper.
// Built with g++ -std=c++11 against librslf_hip.so.  Reads <dir>/volume.f32, a [3][17][150][3] float field in [0, 1) that
// tests/test_gpu_cpp_scores.py wrote, runs the pile computer on it and writes the rows the getter returns -- of every
// scanline, and of a window -- for the pytest side, which compares them with the Python getter's tensor.  The object
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
        rslfx::Depth1DComputer_pile<3> pile(ctx, ptrs.data(), false, V, S, U, 0, -2.0f, 5.0f, D, -1, 1.0f);
        bool refused = false;
        try {
            pile.get_scores();   // before run() there is nothing to show
        } catch (const rslfx::Error& e) {
            refused = e.status == RSLF_ERR_INVALID_ARG;
        }
        if (!refused)
            return 1;
        pile.run();
        const std::vector<float> rows = pile.get_scores();
        if (rows.size() != (size_t)V * U * D)
            return 1;
        dump(dir + "/scores.f32", rows);
        dump(dir + "/scores_row1.f32", pile.get_scores(1, 1));
        dump(dir + "/mask.u8", pile.m_edge_confidence_mask_v_u);
        dump(dir + "/idx.i32", pile.m_depth_idx_v_u);
        refused = false;
        try {
            pile.get_scores(2, 2);   // not a window of three scanlines
        } catch (const rslfx::Error& e) {
            refused = e.status == RSLF_ERR_INVALID_ARG;
        }
        if (!refused)
            return 1;

        // the MultiContext form keeps no volume on a device: it throws, naming the reason
        rslfx::MultiContext multi(std::vector<int>(2, 0));
        rslfx::Depth1DComputer_pile<3> shared(multi, ptrs.data(), false, V, S, U, 0, -2.0f, 5.0f, D, -1, 1.0f);
        shared.run();
        if (shared.m_depth_idx_v_u != pile.m_depth_idx_v_u)
            return 1;
        bool threw = false;
        try {
            shared.get_scores();
        } catch (const std::invalid_argument& e) {
            threw = std::string(e.what()).find("MultiContext") != std::string::npos;
        }
        std::printf("host scores: %s\n", threw ? "ok" : "FAILED: the MultiContext form did not throw std::invalid_argument");
        return threw ? 0 : 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 3;
    }
}
