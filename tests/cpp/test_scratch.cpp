// GrowBuf (rslf_scratch.hpp), the library's one owning buffer type, with a counting allocator in place of the device's:
// compiled with g++ alone and run under AddressSanitizer / UBSan (tests/test_plan_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "rslf_scratch.hpp"

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

namespace {

// Counts calls, logs their order ('a' / 'f'), tracks the bytes live, and fails on request.
struct Counting {
    static int allocs, frees, fail_allocs, fail_frees;
    static size_t live, peak;
    static std::string log;
    static std::vector<std::pair<void*, size_t>> blocks;
    static int alloc(size_t bytes, void** out)
    {
        if (fail_allocs > 0) {
            fail_allocs--;
            return 2;
        }
        *out = std::malloc(bytes);
        blocks.emplace_back(*out, bytes);
        allocs++, live += bytes, log += 'a';
        peak = live > peak ? live : peak;
        return 0;
    }
    static int free(void* p)
    {
        if (fail_frees > 0) {
            fail_frees--;
            return 3;
        }
        for (size_t i = 0; i < blocks.size(); i++)
            if (blocks[i].first == p) {
                live -= blocks[i].second;
                blocks.erase(blocks.begin() + (long)i);
                std::free(p);
                frees++, log += 'f';
                return 0;
            }
        std::printf("FAILED: free of a pointer the allocator never gave out (or gave out and took back)\n");
        std::exit(1);
    }
};
int Counting::allocs = 0, Counting::frees = 0, Counting::fail_allocs = 0, Counting::fail_frees = 0;
size_t Counting::live = 0, Counting::peak = 0;
std::string Counting::log;
std::vector<std::pair<void*, size_t>> Counting::blocks;

using Buf = rslf::GrowBuf<Counting>;

struct Dev {   // like rslf_multi::Dev: held in a vector, reset by assignment
    Buf planes[2];
    Buf arena;
};

}  // namespace

int main()
{
    {   // grow-only; free before allocate; fresh exactly on new storage
        Buf b;
        CHECK(b.get() == nullptr && b.capacity() == 0);
        rslf::Reserved r = b.reserve(0);   // nothing asked for: nothing made
        CHECK(r.err == 0 && !r.fresh && b.get() == nullptr && Counting::allocs == 0);
        r = b.reserve(100);
        CHECK(r.err == 0 && r.fresh && b.get() && b.capacity() == 100 && Counting::log == "a");
        b.as<unsigned char>()[99] = 7;   // (ASan checks the extent)
        void* p = b.get();
        r = b.reserve(40);   // smaller: neither frees nor allocates, contents stay
        CHECK(r.err == 0 && !r.fresh && b.get() == p && b.capacity() == 100 && Counting::log == "a");
        r = b.reserve(100);
        CHECK(r.err == 0 && !r.fresh && b.get() == p && b.as<unsigned char>()[99] == 7);
        r = b.reserve(101);   // larger: the old storage goes FIRST
        CHECK(r.err == 0 && r.fresh && b.capacity() == 101 && Counting::log == "afa");
        CHECK(Counting::peak == 101);   // never old + new together
        CHECK(b.as<int>() == static_cast<int*>(b.get()));

        // stale: storage kept, the next reserve reports fresh once
        p = b.get();
        b.mark_stale();
        r = b.reserve(8);
        CHECK(r.err == 0 && r.fresh && b.get() == p && b.capacity() == 101 && Counting::log == "afa");
        r = b.reserve(8);
        CHECK(!r.fresh);
        b.mark_stale();
        r = b.reserve(200);   // stale and too small: new storage, fresh once
        CHECK(r.fresh && b.capacity() == 200 && Counting::log == "afafa");
        CHECK(!b.reserve(200).fresh);
    }
    CHECK(Counting::log == "afafaf" && Counting::live == 0);   // the destructor freed the last one
    {   // an empty buffer has nothing to go stale
        Buf b;
        b.mark_stale();
        CHECK(!b.reserve(0).fresh && Counting::log == "afafaf");
    }

    {   // a failed allocation leaves {nullptr, 0}; the next reserve retries
        Buf b;
        CHECK(b.reserve(16).err == 0);
        Counting::fail_allocs = 1;
        rslf::Reserved r = b.reserve(32);
        CHECK(r.err == 2 && !r.fresh && b.get() == nullptr && b.capacity() == 0 && Counting::live == 0);
        r = b.reserve(8);   // smaller than what it once held: still has to allocate
        CHECK(r.err == 0 && r.fresh && b.capacity() == 8);
        // a failed free leaves the buffer as it was (and is reported)
        void* p = b.get();
        Counting::fail_frees = 1;
        r = b.reserve(64);
        CHECK(r.err == 3 && !r.fresh && b.get() == p && b.capacity() == 8);
        CHECK(b.reserve(64).err == 0 && b.capacity() == 64);
    }
    CHECK(Counting::live == 0 && Counting::allocs == Counting::frees);

    {   // moves leave the source empty; move assignment frees what the target held
        Buf a;
        CHECK(a.reserve(24).err == 0);
        void* p = a.get();
        Buf b(std::move(a));
        CHECK(a.get() == nullptr && a.capacity() == 0 && b.get() == p && b.capacity() == 24);
        CHECK(a.reserve(0).err == 0 && a.get() == nullptr);
        Buf c;
        CHECK(c.reserve(48).err == 0);
        const int frees = Counting::frees;
        c = std::move(b);
        CHECK(Counting::frees == frees + 1 && b.get() == nullptr && b.capacity() == 0 && c.get() == p && c.capacity() == 24);
        c.mark_stale();
        Buf d(std::move(c));   // staleness travels with the storage
        CHECK(d.reserve(1).fresh && !c.reserve(0).fresh);
        std::swap(a, d);       // (fine-to-coarse swaps the raw volumes of two levels)
        CHECK(a.get() == p && d.get() == nullptr);

        std::vector<Dev> devs(2);
        CHECK(devs[1].planes[0].reserve(10).err == 0 && devs[1].planes[1].reserve(10).err == 0 && devs[1].arena.reserve(99).err == 0);
        devs.resize(5);        // reallocation moves the elements
        CHECK(devs[1].arena.capacity() == 99 && devs[4].arena.get() == nullptr);
        const size_t live = Counting::live;
        devs[1] = Dev();       // multi_free_dev
        CHECK(Counting::live == live - 119 && devs[1].planes[0].get() == nullptr);
        CHECK(devs[0].arena.reserve(5).err == 0);   // one left for the vector's destructor
    }
    CHECK(Counting::live == 0 && Counting::allocs == Counting::frees);

    {   // The fuzz-found order (tests/test_gpu_sweep2d.py::test_scratch_reuse_across_shapes): S*V*U shrinks while V*U grows.
        // Two buffers, each with its own capacity, always hold what was asked of them (one capacity in S*V*U entries for
        // both would stop growing after the first shape and leave the plane at 200 floats).
        const int shapes[5][3] = {{13, 2, 100}, {5, 4, 110}, {3, 16, 40}, {2, 20, 45}, {1, 30, 50}};   // S, V, U
        Buf winner, filtered;
        const int allocs = Counting::allocs;
        for (const int* s : shapes) {
            const size_t n = (size_t)s[0] * s[1] * s[2], plane = (size_t)s[1] * s[2];
            CHECK(winner.reserve(n * sizeof(int)).err == 0 && filtered.reserve(plane * sizeof(float)).err == 0);
            CHECK(winner.capacity() >= n * sizeof(int) && filtered.capacity() >= plane * sizeof(float));
            winner.as<int>()[n - 1] = 1;   // the last element each kernel would touch (ASan checks it)
            filtered.as<float>()[plane - 1] = 1.0f;
        }
        CHECK(winner.capacity() == (size_t)13 * 2 * 100 * sizeof(int));   // S*V*U only shrank: allocated once
        CHECK(filtered.capacity() == (size_t)30 * 50 * sizeof(float));    // V*U grew every time: 200, 440, 640, 900, 1500
        CHECK(Counting::allocs == allocs + 1 + 5);
    }
    CHECK(Counting::live == 0 && Counting::allocs == Counting::frees && Counting::blocks.empty());
    std::printf("scratch tests ok (%d allocations, %d frees)\n", Counting::allocs, Counting::frees);
    return 0;
}
