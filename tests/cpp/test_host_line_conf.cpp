// rslfx::Depth2DComputer with par_line_confidence_mode = RSLF_LINE_CONF_GATE through include/rslf_hip.hpp, compiled with
// g++ against librslf_hip.so (tests/test_gpu_line_conf.py compares the planes it writes with tests/line_conf_ref.py).
//   test_host_line_conf DIR V S U D THRESHOLD     reads DIR/input.f32 ([V][S][U] float32, already in [0, 1])
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
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s DIR V S U D THRESHOLD\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int V = std::atoi(argv[2]), S = std::atoi(argv[3]), U = std::atoi(argv[4]), D = std::atoi(argv[5]);
    const float thr = std::strtof(argv[6], nullptr);
    std::vector<float> flat((size_t)V * S * U);
    FILE* f = std::fopen((dir + "/input.f32").c_str(), "rb");
    if (!f || std::fread(flat.data(), sizeof(float), flat.size(), f) != flat.size()) {
        std::perror("input.f32");
        return 2;
    }
    std::fclose(f);
    std::vector<const void*> ptrs(V);
    for (int v = 0; v < V; v++)
        ptrs[v] = flat.data() + (size_t)v * S * U;
    try {
        rslfx::Context ctx(0);
        rslfx::Depth1DParameters par;
        if (par.par_line_confidence_mode != RSLF_LINE_CONF_OFF)
            return 3;
        par.par_line_confidence_mode = RSLF_LINE_CONF_GATE;
        par.par_line_score_threshold = thr;
        rslfx::Depth2DComputer<1> d2(ctx, ptrs.data(), false, V, S, U, 0, -1.0f, 1.0f, D, 1.0f, par);
        d2.run();
        dump(dir + "/lc_depth.f32", d2.get_depths_s_v_u());
        dump(dir + "/lc_mask.u8", d2.m_edge_confidence_mask_s_v_u);
        dump(dir + "/lc_Ce.f32", d2.m_edge_confidence_s_v_u);
        dump(dir + "/lc_Cd.f32", d2.m_disp_confidence_s_v_u);
        dump(dir + "/lc_Cl.f32", d2.m_line_confidence_s_v_u);
        std::vector<uint8_t> lut(768);
        for (int i = 0; i < 256; i++)
            lut[3 * i] = (uint8_t)i, lut[3 * i + 1] = (uint8_t)(255 - i), lut[3 * i + 2] = (uint8_t)(i ^ 0x55);
        dump(dir + "/lc_lut.u8", lut);
        dump(dir + "/lc_map.u8", d2.get_disparity_map(-1, lut.data()));   // painted under C_l > threshold (dc.hpp:883)
        std::printf("line confidence: Depth2DComputer scanned %lld px\n", (long long)d2.stats.pixels_scanned);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
