// powtab.hpp — g^e through a two-level power table, for any field element g
// and exponents e < n <= 2^28:
//   g^e = T1[e & 0xfff] * T2[e >> 12]      (one multiply, two cached loads)
// T1 holds g^j, j < min(n, 4096); T2 holds scale * g^(4096 j), j <
// ceil(n / 4096). Both live in one run of pow_table_elems(n) elements
// (scratch.hpp), and T2 starts at element POW_LOW whatever n is (T1 entries
// from n up are neither written nor read). The NTT's twiddle and coset
// factors and the permutation argument's row powers resolve through it.
#pragma once
#include "ff.hpp"
#include "scratch.hpp"

#define POW_LOW_MASK (POW_LOW - 1u)

struct PowTable { const fp256 *T1, *T2; };
// o = g^e, multiplied in F (the tables' bytes do not depend on the multiply)
template <class F>
__device__ __forceinline__ void pow_lookup(fp256& o, const PowTable& t,
                                           uint64_t e) {
    ff_mul<F>(o, t.T1[(uint32_t)e & POW_LOW_MASK], t.T2[e >> POW_LOW_BITS]);
}

struct DeviceState;
// powtab.hip — both enqueue one launch on ds.stream and do not synchronize.
// The table of g for exponents < n (1 <= n <= 2^28) into the
// pow_table_elems(n) elements at dst; returns its two halves. A null scale
// is 1.
PowTable pow_tables_build(DeviceState& ds, const fp256& g, const fp256* scale,
                          uint64_t n, fp256* dst);
// out[j] = g^j, j < count, 1 <= count <= 2^28
void pow_linear_build(DeviceState& ds, const fp256& g, fp256* out,
                      uint32_t count);
