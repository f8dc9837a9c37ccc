// include/rslf_hip.hpp on a CV_16U light field, the way the reference's demos hold one (a Vec<Mat> of 16-bit EPIs;
// RSLightFields/tests/test_fine_to_coarse.cpp reads raw 16-bit TIFFs): Depth1DComputer_pile<1> and FineToCoarse<1>
// from uint16 pointers (rslfx::InputType::U16).  Built with g++ -std=c++11 against librslf_hip.so by
// tests/test_gpu_u16.py, which writes the input and compares the planes written here with the Python u16 results.
//   test_host_wrapper_u16 <dir> V S U      reads <dir>/input.u16 ([V][S][U] uint16), writes <dir>/pile_* and f2c_*
#include <cstdio>
#include <cstdlib>
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
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s <dir> V S U\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int V = std::atoi(argv[2]), S = std::atoi(argv[3]), U = std::atoi(argv[4]);
    // one separately allocated buffer per scanline, as a Vec<Mat> holds them
    std::vector<std::vector<uint16_t> > epis((size_t)V, std::vector<uint16_t>((size_t)S * U));
    FILE* f = std::fopen((dir + "/input.u16").c_str(), "rb");
    if (!f)
        return 3;
    for (int v = 0; v < V; v++)
        if (std::fread(epis[(size_t)v].data(), sizeof(uint16_t), (size_t)S * U, f) != (size_t)S * U)
            return 4;
    std::fclose(f);
    std::vector<const void*> ptrs((size_t)V);
    for (int v = 0; v < V; v++)
        ptrs[(size_t)v] = epis[(size_t)v].data();
    try {
        rslfx::Context ctx(0);
        rslfx::Depth1DComputer_pile<1> pile(ctx, ptrs.data(), rslfx::InputType::U16, V, S, U, 0, -1.0f, 2.0f, 16);
        pile.run();
        dump(dir + "/pile_Ce.f32", pile.m_edge_confidence_v_u);
        dump(dir + "/pile_mask.u8", pile.m_edge_confidence_mask_v_u);
        dump(dir + "/pile_depth.f32", pile.m_best_depth_v_u);
        dump(dir + "/pile_idx.i32", pile.m_depth_idx_v_u);
        dump(dir + "/pile_score.f32", pile.m_score_v_u);
        dump(dir + "/pile_scale.f32", std::vector<float>(1, pile.epi_scale_factor()));
        rslfx::FineToCoarse<1> f2c(ctx, ptrs.data(), rslfx::InputType::U16, V, S, U, 0, -1.0f, 1.0f, 9);
        f2c.run();
        std::vector<float> map;
        std::vector<uint8_t> valid;
        f2c.get_results(map, valid);
        dump(dir + "/f2c_map.f32", map);
        dump(dir + "/f2c_valid.u8", valid);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
