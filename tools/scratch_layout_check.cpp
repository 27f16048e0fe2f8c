// scratch_layout_check — stand-alone host check of how the synchronous device
// calls carve up the call arena (spectre_amd/csrc/scratch.hpp): for every
// user's sequence of extents and a sweep of sizes from 1 to 2^28, every
// offset is 256-aligned, no two extents share a byte, every extent ends
// inside the total that the call reserves, and the total does not wrap. The
// sequences below are the ones the host code adds, in its order; a call with
// a single extent reserves count * sizeof directly, which the same checks
// bound. Meant to be built with a sanitizer and run on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I spectre_amd/csrc
//       tools/scratch_layout_check.cpp -o scratch_layout_check
#include "poly_levels.hpp"
#include "scratch.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

struct fp256 { uint32_t l[8]; };  // the size of the library's field element

static int fails = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAIL %s (%s n=%llu)\n", #c, who,                 \
                        (unsigned long long)n);                           \
            fails++;                                                      \
        }                                                                 \
    } while (0)

// One call's layout as it is built, with the byte length of every extent.
struct Call {
    ScratchLayout lay;
    std::vector<uint64_t> off, len;
    template <typename T>
    void add(uint64_t count) {
        off.push_back(lay.add<T>(count));
        len.push_back(count * sizeof(T));
    }
};

// limit: more than any call can ask for (the lookup at 2^28 rows takes 35 GiB
// and its hipCUB temp storage; a gate program of 2^32 constants 128 GiB), far
// below a wrap
static void check(const char* who, uint64_t n, const Call& c) {
    const uint64_t limit = 1ull << 38;
    uint64_t end = 0;  // of the extents before this one
    for (size_t i = 0; i < c.off.size(); i++) {
        CHECK(c.off[i] % SCRATCH_ALIGN == 0);
        CHECK(c.off[i] >= end);  // in order, so: no overlap with any earlier
        CHECK(c.len[i] <= limit && c.off[i] <= limit);
        end = c.off[i] + c.len[i];
        CHECK(end <= c.lay.total);
    }
    CHECK(c.lay.total % SCRATCH_ALIGN == 0);
    CHECK(c.lay.total <= limit);
    CHECK(c.lay.total - end < SCRATCH_ALIGN);  // and no more than that
}

static void check_pow_table(uint64_t n) {
    const char* who = "pow_table_elems";
    const uint64_t e = pow_table_elems(n);
    CHECK(e == POW_LOW + (n + POW_LOW - 1) / POW_LOW);
    // the last exponent n - 1 reads T2 at element POW_LOW + ((n - 1) >> 12)
    CHECK(POW_LOW + ((n - 1) >> POW_LOW_BITS) < e);
}

static void check_size(uint64_t n) {
    check_pow_table(n);
    {  // perm.hip: the row-power table of fr_powers and of the terms
        Call c;
        c.add<fp256>(pow_table_elems(n));
        check("perm", n, c);
    }
    {  // lookup.hip over n rows; temp storage of a few sizes, none included
        for (uint64_t tmp : {0ull, 1ull, 256ull, 9ull * n + 4097ull}) {
            Call c;
            c.add<fp256>(2 * n);
            c.add<fp256>(n);
            c.add<uint64_t>(2 * n);
            c.add<uint32_t>(7 * n);
            c.add<uint32_t>(9);
            c.add<uint8_t>(tmp);
            check("lookup", n, c);
        }
    }
    for (uint64_t tile = 256; tile <= 1024; tile += 256) {  // poly.hip
        {
            Call c;
            c.add<fp256>((n + tile - 1) / tile + 1);
            check("grand product", n, c);
        }
        const PolyLevels ev = poly_levels(n, tile, 1, 1);
        const PolyLevels dv = poly_levels(n, tile, tile, 0);
        const char* who = "poly levels";
        CHECK(ev.ok && dv.ok);
        // one partial vector per polynomial and point: fr_poly_eval has one
        // polynomial, fr_poly_eval_batch up to 32
        for (uint64_t npolys : {1ull, 2ull, 31ull, 32ull}) {
            for (uint64_t npoints = 1; npoints <= 8; npoints++) {
                Call c;
                c.add<fp256>(npolys * npoints * ev.total);
                check("poly eval", n, c);
            }
        }
        // a remainder slot per root: fr_poly_div_linear has one root,
        // fr_poly_div_roots up to 8
        for (uint64_t nroots = 1; nroots <= 8; nroots++) {
            Call c;
            c.add<fp256>(dv.total + nroots);
            check("poly div", n, c);
        }
    }
}

int main() {
    const uint64_t kMaxN = 1ull << 28;
    std::vector<uint64_t> ns;
    for (uint64_t n = 1; n <= 4100; n++) ns.push_back(n);
    for (uint64_t p = 8192; p <= kMaxN; p *= 2)
        for (int d = -1; d <= 1; d++) ns.push_back(p + d);
    for (uint64_t n = 4099; n < kMaxN; n = n * 3 + 1) ns.push_back(n);
    for (uint64_t n : ns)
        if (n <= kMaxN) check_size(n);
    // ntt.hip: n a power of two, tmp and, with a coset generator, its table
    for (uint32_t log_n = 1; log_n <= 28; log_n++) {
        const uint64_t n = 1ull << log_n;
        for (int coset = 0; coset < 2; coset++) {
            Call c;
            c.add<fp256>(n);
            c.add<fp256>(coset ? pow_table_elems(n) : 0);
            check(coset ? "coset ntt" : "ntt", n, c);
        }
    }
    // gate.hip: [col ptrs][constants][program of 3-word ops], any counts
    const unsigned long long kMax32 = 0xffffffffull;
    for (uint64_t ncols : {0ull, 1ull, 31ull, 32ull, 33ull, 65536ull, kMax32})
        for (uint64_t nconst : {0ull, 1ull, 7ull, 8ull, 9ull, kMax32})
            for (uint64_t nops : {1ull, 21ull, 22ull, 1ull << 20, kMax32}) {
                Call c;
                c.add<fp256*>(ncols);
                c.add<fp256>(nconst);
                c.add<uint32_t>(3 * nops);
                check("gate", ncols + nconst + nops, c);
            }
    if (fails) std::printf("scratch_layout_check: %d failures\n", fails);
    else std::printf("scratch_layout_check: ok\n");
    return fails ? EXIT_FAILURE : EXIT_SUCCESS;
}
