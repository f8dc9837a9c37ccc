// rslfx::FineToCoarse with set_line_confidence_mode(RSLF_LINE_CONF_GATE) through include/rslf_hip.hpp, compiled with g++
// against librslf_hip.so (tests/test_gpu_cpp_f2c_line_conf.py compares what it writes with tests/f2c_line_conf_ref.py and
// with the Python getter).
//   test_host_f2c_line_conf DIR V S U D THRESHOLD     reads DIR/input.f32 ([V][S][U] float32, raw values)
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
        par.par_line_score_threshold = thr;
        rslfx::FineToCoarse<1> f2c(ctx, ptrs.data(), false, V, S, U, 0, -1.0f, 1.0f, D, -1.0f, par);
        bool threw = false;
        try {
            f2c.set_line_confidence_mode(3);
        } catch (const rslfx::Error&) {
            threw = true;
        }
        if (!threw || !f2c.get_depths_pyr().empty())
            return 3;
        f2c.set_line_confidence_mode(RSLF_LINE_CONF_GATE);
        f2c.run();
        const int P = f2c.pyramid_depth();
        if ((int)f2c.pyramid_dims().size() != P || (int)f2c.get_line_confidence_pyr().size() != P)
            return 4;
        std::vector<uint8_t> lut(768);
        for (int i = 0; i < 256; i++)
            lut[3 * i] = (uint8_t)i, lut[3 * i + 1] = (uint8_t)(255 - i), lut[3 * i + 2] = (uint8_t)(i ^ 0x55);
        dump(dir + "/f2c_lut.u8", lut);
        const std::vector<std::vector<uint8_t> > pyr = f2c.get_coloured_depth_pyr(-1, lut.data());
        FILE* d = std::fopen((dir + "/f2c_dims.txt").c_str(), "w");
        for (int l = 0; l < P; l++) {
            const std::string tag = dir + "/f2c_l" + std::to_string(l);
            std::fprintf(d, "%d %d\n", f2c.pyramid_dims()[l].first, f2c.pyramid_dims()[l].second);
            dump(tag + "_Cl.f32", f2c.get_line_confidence_pyr()[l]);
            dump(tag + "_valid.u8", f2c.get_validity_pyr()[l]);
            dump(tag + "_depth.f32", f2c.get_depths_pyr()[l]);
            dump(tag + "_pyr.u8", pyr[l]);
        }
        std::fclose(d);
        std::vector<float> map;
        std::vector<uint8_t> valid;
        f2c.get_results(map, valid);
        dump(dir + "/f2c_map.f32", map);
        dump(dir + "/f2c_valid.u8", valid);
        std::printf("fine-to-coarse with line confidence: %d levels, %lld px scanned\n", P, (long long)f2c.stats.pixels_scanned);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
