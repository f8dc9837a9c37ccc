// rslfx::Depth2DComputer::set_peaks / get_peaks (include/rslf_hip.hpp): the 2-D sweep's peaks mode through the C++11 host
// wrapper.  Built with g++ -std=c++11 against librslf_hip.so.  Reads <dir>/sweep.f32, the [6][5][80] planted field written by
// tests/test_gpu_cpp_sweep_peaks.py; runs the class with the mode off and on -- alone and with the sub-grid mode -- and writes
// the planes out for the pytest side, which compares them with the Python object's.  The mode changes no other plane; an
// object built on a MultiContext must refuse it with std::invalid_argument.
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
static bool throws_invalid(Obj& o, bool getter)
{
    try {
        if (getter)
            (void)o.get_peaks();
        else
            o.set_peaks(true);
    } catch (const std::invalid_argument& e) {
        return std::string(e.what()).find("MultiContext") != std::string::npos;
    }
    return false;
}

static int fail(const char* what)
{
    std::printf("host sweep peaks: FAILED: %s\n", what);
    return 1;
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    try {
        rslfx::Context ctx(0);
        rslfx::MultiContext multi(std::vector<int>(2, 0));
        const int V = 6, S = 5, U = 80, D = 9;
        const size_t n = (size_t)S * V * U;
        const std::vector<float> field = load(dir + "/sweep.f32", (size_t)V * S * U);
        std::vector<const void*> ptrs(V);
        for (int v = 0; v < V; v++)
            ptrs[v] = field.data() + (size_t)v * S * U;
        rslfx::Depth2DComputer<1> comp(ctx, ptrs.data(), false, V, S, U, 0, -2.0f, 2.0f, D, 1.0f);
        comp.run();   // default off
        const std::vector<float> grid = comp.get_depths_s_v_u(), grid_Cd = comp.m_disp_confidence_s_v_u;
        bool refused = false;
        try {
            (void)comp.get_peaks();
        } catch (const std::invalid_argument&) {
            refused = true;
        }
        if (!refused)
            return fail("get_peaks without set_peaks(true) did not throw");
        comp.set_peaks(true);
        comp.run();
        const rslfx::Depth2DComputer<1>::Peaks& pk = comp.get_peaks();
        if (pk.idx.size() != n || pk.score.size() != n || pk.runner_idx.size() != n || pk.runner_score.size() != n)
            return fail("the four planes are not [S][V][U]");
        if (!same_bits(comp.get_depths_s_v_u(), grid) || !same_bits(comp.m_disp_confidence_s_v_u, grid_Cd))
            return fail("the mode changed a plane the sweep had before");
        size_t winners = 0, runners = 0, none = 0;
        for (size_t k = 0; k < n; k++) {
            winners += pk.idx[k] >= 0;
            runners += pk.runner_idx[k] >= 0;
            none += pk.idx[k] == -1 && pk.score[k] == 0.0f && pk.runner_idx[k] == -1 && pk.runner_score[k] == 0.0f;
            if (pk.idx[k] >= D || pk.runner_idx[k] >= D || (pk.runner_idx[k] >= 0 && pk.idx[k] < 0) ||
                (pk.runner_idx[k] >= 0 && pk.runner_score[k] > pk.score[k]))
                return fail("a pixel's peaks are not a winner and a runner-up of a row");
        }
        if (winners < 1000 || runners < 10 || none < 10)
            return fail("too few winners, runners-up or untouched pixels");
        dump(dir + "/pk_idx.i32", pk.idx);
        dump(dir + "/pk_score.f32", pk.score);
        dump(dir + "/pk_runner_idx.i32", pk.runner_idx);
        dump(dir + "/pk_runner_score.f32", pk.runner_score);
        dump(dir + "/pk_depth.f32", comp.get_depths_s_v_u());
        comp.set_subgrid(true);   // the two modes together
        comp.run();
        dump(dir + "/pk_sub_idx.i32", comp.get_peaks().idx);
        dump(dir + "/pk_sub_runner_score.f32", comp.get_peaks().runner_score);
        dump(dir + "/pk_sub_depth.f32", comp.get_depths_s_v_u());
        comp.set_subgrid(false);
        comp.set_peaks(false);    // back off: the planes of the plain run
        comp.run();
        if (!same_bits(comp.get_depths_s_v_u(), grid))
            return fail("the planes after set_peaks(false) are not the plain run's");
        rslfx::Depth2DComputer<1> shared(multi, ptrs.data(), false, V, S, U, 0, -2.0f, 2.0f, D, 1.0f);
        if (!throws_invalid(shared, false) || !throws_invalid(shared, true))
            return fail("Depth2DComputer on a MultiContext did not throw std::invalid_argument");
        shared.set_peaks(false);   // off is always accepted
        std::printf("host sweep peaks: ok\n");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "FAILED: %s\n", e.what());
        return 3;
    }
}
