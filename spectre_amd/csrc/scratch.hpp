// scratch.hpp — how one synchronous device call carves up the per-device
// call arena (DeviceState::d_call, internal.hpp): pure host arithmetic, no
// HIP, so a plain C++ program can check every user's layout under a
// sanitizer (tools/scratch_layout_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

// hipMalloc's own alignment, and what hipCUB temp storage asks for
#define SCRATCH_ALIGN 256ull

// A call adds its extents in turn and reserves `total` bytes once (a call
// with a single extent has nothing to lay out and reserves its bytes). All in
// 64 bits: the largest user (lookup.hip at 2^28 rows) adds 7 * 2^28 words
// and 3 * 2^28 elements.
struct ScratchLayout {
    uint64_t total = 0;  // bytes, a multiple of SCRATCH_ALIGN
    // byte offset of `count` objects of type T; an empty extent takes nothing
    template <typename T>
    uint64_t add(uint64_t count) {
        const uint64_t off = total;
        total += (count * sizeof(T) + SCRATCH_ALIGN - 1) & ~(SCRATCH_ALIGN - 1);
        return off;
    }
};

// Elements of the two-level power table (powtab.hpp) for exponents < n:
// T1 takes POW_LOW slots whatever n is, T2 one per 4096 exponents.
#define POW_LOW_BITS 12
#define POW_LOW (1u << POW_LOW_BITS)
inline uint64_t pow_table_elems(uint64_t n) {
    return POW_LOW + ((n + POW_LOW - 1) >> POW_LOW_BITS);
}
