// The dilation along u through the C++11 host wrapper (include/rslf_hip.hpp): set_u_dilation(2, RSLF_DILATE_CUBIC) on
// rslfx::Depth1DComputer_pile and rslfx::Depth2DComputer, the undilated getters, and the two forms that throw -- an object
// built on a MultiContext and FineToCoarse.  Built with g++ -std=c++11 against librslf_hip.so.  Reads <dir>/input.f32, a
// synthetic field [5][7][80] in [0, 1), and the planes the Python classes computed with u_dilation = 2
// (tests/test_gpu_cpp_dilate.py wrote them): every plane must hold the same bytes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "rslf_hip.hpp"

typedef rslfx::Depth1DComputer_pile<1> Pile;
typedef rslfx::Depth2DComputer<1> Sweep;
typedef rslfx::FineToCoarse<1> F2c;

template <typename T>
static std::vector<T> load(const std::string& path, size_t n)
{
    std::vector<T> v(n);
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f || std::fread(v.data(), sizeof(T), n, f) != n) {
        std::perror(path.c_str());
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

template <typename T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

template <typename T>
static std::vector<T> every(const std::vector<T>& planes, int dim_u, int factor)   // planes[..., ::factor]
{
    std::vector<T> out;
    for (size_t r = 0; r < planes.size() / dim_u; r++)
        for (int u = 0; u < dim_u; u += factor)
            out.push_back(planes[r * dim_u + u]);
    return out;
}

template <typename Fn>
static bool throws_invalid(Fn fn)
{
    try {
        fn();
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
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

#define EXPECT(cond)                                                           \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("%s:%d: EXPECT failed: %s\n", __FILE__, __LINE__, #cond); \
            rc = 1;                                                            \
        }                                                                      \
    } while (0)

static int run(const std::string& dir)
{
    const int V = 5, S = 7, U = 80, D = 12, F = 2, Ud = F * (U - 1) + 1;
    const std::vector<float> raw = load<float>(dir + "/input.f32", (size_t)V * S * U);
    std::vector<const void*> epis(V);
    for (int v = 0; v < V; v++)
        epis[v] = raw.data() + (size_t)v * S * U;
    rslfx::Context ctx(0);
    int rc = 0;
    rslfx::Depth1DParameters params = rslfx::Depth1DParameters::get_default();

    // ---- Depth1DComputer_pile ---------------------------------------------------------------------------------------------
    {
        const size_t n = (size_t)V * Ud;
        Pile comp(ctx, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D, -1, 1.0f, params);
        EXPECT(comp.get_u_dilation() == 1 && comp.u_dilated() == U && comp.cols() == U);
        EXPECT(refuses([&] { comp.set_u_dilation(0); }) && refuses([&] { comp.set_u_dilation(9); }) && refuses([&] { comp.set_u_dilation(2, 3); }));
        EXPECT(comp.get_u_dilation() == 1 && comp.u_dilated() == U);
        comp.run();
        const std::vector<float> plain = comp.m_best_depth_v_u;
        EXPECT(plain.size() == (size_t)V * U && same_bytes(comp.get_best_depth_undilated(), plain));   // factor 1: the plane itself
        comp.set_u_dilation(F, RSLF_DILATE_CUBIC);
        EXPECT(comp.get_u_dilation() == F && comp.u_dilated() == Ud && comp.cols() == Ud && comp.m_best_depth_v_u.empty());
        EXPECT(refuses([&] { (void)comp.get_best_depth_undilated(); }));   // before run()
        EXPECT(params.par_slope_factor == 1.0f);                          // the caller's object is not modified
        comp.run();
        EXPECT(same_bytes(comp.m_best_depth_v_u, load<float>(dir + "/pile_depth.f32", n)));
        EXPECT(same_bytes(comp.m_edge_confidence_mask_v_u, load<uint8_t>(dir + "/pile_edge_mask.u8", n)));
        EXPECT(same_bytes(comp.m_edge_confidence_v_u, load<float>(dir + "/pile_edge_confidence.f32", n)));
        EXPECT(same_bytes(comp.m_depth_idx_v_u, load<int32_t>(dir + "/pile_depth_idx.i32", n)));
        EXPECT(same_bytes(comp.m_score_v_u, load<float>(dir + "/pile_score.f32", n)));
        EXPECT(same_bytes(comp.m_rbar_v_u, load<float>(dir + "/pile_rbar.f32", n)));
        EXPECT(same_bytes(comp.get_best_depth_undilated(), every(comp.m_best_depth_v_u, Ud, F)));
        EXPECT(same_bytes(comp.get_edge_confidence_mask_undilated(), every(comp.m_edge_confidence_mask_v_u, Ud, F)));
        EXPECT(comp.get_best_depth_undilated().size() == (size_t)V * U);
        // factor 1 puts the source back: the first run's plane
        comp.set_u_dilation(1);
        EXPECT(comp.u_dilated() == U);
        comp.run();
        EXPECT(same_bytes(comp.m_best_depth_v_u, plain));
    }

    // ---- Depth2DComputer --------------------------------------------------------------------------------------------------
    {
        const size_t n = (size_t)S * V * Ud;
        Sweep comp(ctx, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D, 1.0f, params);
        comp.set_u_dilation(F, RSLF_DILATE_CUBIC);
        EXPECT(comp.get_u_dilation() == F && comp.u_dilated() == Ud);
        comp.run();
        EXPECT(same_bytes(comp.get_depths_s_v_u(), load<float>(dir + "/sweep_depth.f32", n)));
        EXPECT(same_bytes(comp.m_edge_confidence_mask_s_v_u, load<uint8_t>(dir + "/sweep_edge_mask.u8", n)));
        EXPECT(same_bytes(comp.m_edge_confidence_s_v_u, load<float>(dir + "/sweep_edge_confidence.f32", n)));
        EXPECT(same_bytes(comp.m_rbar_s_v_u, load<float>(dir + "/sweep_rbar.f32", n)));
        EXPECT(same_bytes(comp.get_valid_depths_mask_s_v_u(), load<uint8_t>(dir + "/sweep_valid.u8", n)));
        EXPECT(same_bytes(comp.get_depths_undilated(), every(comp.get_depths_s_v_u(), Ud, F)));
        EXPECT(same_bytes(comp.get_valid_depths_mask_undilated(), every(comp.get_valid_depths_mask_s_v_u(), Ud, F)));
        EXPECT(comp.get_depths_undilated().size() == (size_t)S * V * U);
        // the getters work in the dilated frame with the scaled slope factor: the agreement counts Python read
        const rslfx::Consistency cs = comp.get_consistency();
        EXPECT(same_bytes(cs.agree, load<int32_t>(dir + "/sweep_agree.i32", n)));
        // the line confidence takes no slope factor
        rslfx::Depth1DParameters lc = params;
        lc.par_line_confidence_mode = RSLF_LINE_CONF_AS_BUILT;
        Sweep with_lc(ctx, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D, 1.0f, lc);
        with_lc.set_u_dilation(F);
        EXPECT(refuses([&] { with_lc.run(); }));
    }

    // ---- the two throwing forms ---------------------------------------------------------------------------------------------
    {
        rslfx::MultiContext multi(std::vector<int>(1, 0));
        Pile on_multi(multi, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D, -1, 1.0f);
        EXPECT(throws_invalid([&] { on_multi.set_u_dilation(2); }));
        Sweep sweep_on_multi(multi, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D, 1.0f);
        EXPECT(throws_invalid([&] { sweep_on_multi.set_u_dilation(2, RSLF_DILATE_LANCZOS3); }));
        F2c f2c(ctx, epis.data(), false, V, S, U, 0, -1.0f, 1.0f, D, 1.0f);
        EXPECT(throws_invalid([&] { f2c.set_u_dilation(2); }));
        f2c.set_u_dilation(1);   // nothing to do
    }
    return rc;
}

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::printf("usage: %s <dir>\n", argv[0]);
        return 2;
    }
    try {
        const int rc = run(argv[1]);
        std::printf(rc ? "host dilate: FAILED\n" : "host dilate: ok\n");
        return rc;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 3;
    }
}
