// The host-side decisions of the 2-D sweep's sub-grid mode (rslf_plan_subgrid.hpp: which form of the refinement a visit
// queues, the list form's fixed grid, the planes' sizes), compiled with g++ alone and run under AddressSanitizer / UBSan
// (tests/test_sweep_subgrid_cpu.py).
#include <cstdio>
#include <cstdlib>

#include "rslf_plan_subgrid.hpp"

using namespace rslf::plan;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

int main()
{
    const long long small = 6 * 80, c3 = 540ll * 960, limit = 2147483647ll;

    // mode off: no visit refines, whatever else holds
    for (int first = 0; first < 2; first++)
        for (int listed = 0; listed < 2; listed++)
            for (int hook = 0; hook < 2; hook++)
                CHECK(sweep_subgrid_form(false, first, listed, hook, small) == kSubgridNone);

    // mode on: the list form iff the visit's scan took the previous apply pass's packed list
    CHECK(sweep_subgrid_form(true, true, false, 1, small) == kSubgridDense);    // the first visit: nothing is listed yet
    CHECK(sweep_subgrid_form(true, true, true, 1, small) == kSubgridDense);     // first wins over a stale `listed`
    CHECK(sweep_subgrid_form(true, false, true, 1, small) == kSubgridList);     // a sparse visit
    CHECK(sweep_subgrid_form(true, false, true, 1, c3) == kSubgridList);
    CHECK(sweep_subgrid_form(true, false, false, 1, small) == kSubgridDense);   // "force_packed" = 0: the scan compacted for itself
    CHECK(sweep_subgrid_form(true, false, true, 0, small) == kSubgridDense);    // "subgrid_list" = 0
    CHECK(sweep_subgrid_form(true, false, true, 1, limit) == kSubgridList);     // the last plane an int index reaches
    CHECK(sweep_subgrid_form(true, false, true, 1, limit + 1) == kSubgridDense);
    CHECK(sweep_subgrid_form(true, false, true, 1, 65535ll * 65536) == kSubgridDense);

    // the sequence of a five-view sweep: dense, then four listed visits
    {
        bool first = true, listed = false;
        int dense = 0, list = 0;
        for (int visit = 0; visit < 5; visit++) {
            const SubgridForm f = sweep_subgrid_form(true, first, listed, 1, small);
            dense += f == kSubgridDense, list += f == kSubgridList;
            first = false, listed = true;   // what rslf_sweep_visit_finish leaves
        }
        CHECK(dense == 1 && list == 4);
    }

    // the list form's grid: covers the plane's entries where they are few, four workgroups a compute unit where many
    CHECK(subgrid_list_blocks(6, 80, 256) == 2);          // 480 entries at most: two workgroups, the last partial
    CHECK(subgrid_list_blocks(1, 1, 256) == 1);
    CHECK(subgrid_list_blocks(1, 256, 256) == 1 && subgrid_list_blocks(1, 257, 256) == 2);
    CHECK(subgrid_list_blocks(540, 960, 256) == 1024);
    CHECK(subgrid_list_blocks(540, 960, 0) == 1024);      // no device facts: a 256-unit device is assumed
    CHECK(subgrid_list_blocks(540, 960, 8) == 32);
    CHECK(subgrid_list_blocks(46340, 46340, 256) == 1024);   // close to INT32_MAX pixels: no overflow on the way
    CHECK(subgrid_list_blocks(0, 80, 256) == 1 && subgrid_list_blocks(6, -1, 256) == 1);
    // lanes of the whole grid fit an int: the kernel's stride is gridDim.x * 256
    CHECK((long long)subgrid_list_blocks(65535, 32768, 4096) * 256 <= limit);

    // the planes: nothing when off, V * U four-byte values each when on, in size_t
    CHECK(sweep_subgrid_plane_bytes(false, 540, 960) == 0);
    CHECK(sweep_subgrid_plane_bytes(true, 540, 960) == (size_t)540 * 960 * 4);
    CHECK(sweep_subgrid_plane_bytes(true, 65535, 65536) == (size_t)65535 * 65536 * 4);   // > 2^33
    CHECK(sweep_subgrid_plane_bytes(true, 0, 960) == 0 && sweep_subgrid_plane_bytes(true, 540, -3) == 0);

    std::printf("sweep subgrid plan tests ok\n");
    return 0;
}
