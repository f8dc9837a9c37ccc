// The layout of a call's host outputs in the context's output stage (kSharedStageOut; rslf_stack_op.hpp's StagedOut): the
// planes asked for one after the other in the caller's order, each at a multiple of `align`, the others taking no room.
// Host-only like rslf_plan.hpp, which it continues; a pure function, g++ compiles it alone; tested by
// tests/cpp/test_plan_stage.cpp.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace rslf {
namespace plan {

// What stage_layout answers for planes that no address space holds: no size_t is their sum.
constexpr size_t kStageTooLarge = SIZE_MAX;

// offsets[i]: where plane i of bytes[i] bytes starts, for every plane with wanted[i] (the others' entries are left alone).
// align: a power of two -- 1 packs the planes (the consistency check's: 4-byte planes first, then the byte plane), 16 puts
// every plane where the kernels' 16-byte stores may go.  -> the stage's size: the sum of the wanted sizes, each rounded up
// to a multiple of align; 0 with nothing wanted; kStageTooLarge if that sum passes SIZE_MAX - 1.
inline size_t stage_layout(const size_t* bytes, const bool* wanted, int n, size_t align, size_t* offsets)
{
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        if (!wanted[i])
            continue;
        const size_t pad = (align - bytes[i] % align) % align;
        if (bytes[i] > kStageTooLarge - 1 - pad || bytes[i] + pad > kStageTooLarge - 1 - total)
            return kStageTooLarge;
        offsets[i] = total;
        total += bytes[i] + pad;
    }
    return total;
}

}  // namespace plan
}  // namespace rslf
