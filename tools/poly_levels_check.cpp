// poly_levels_check — stand-alone host check of the opening-phase index
// arithmetic (spectre_amd/csrc/poly_levels.hpp): for every tile the library
// accepts and a sweep of n up to 2^28, the level sizes shrink by ceil(./tile)
// down to the stop size, the offsets tile the scratch buffer without gaps or
// overlap, and every index the host code forms from them stays inside the
// total it reserves. Meant to be built with a sanitizer and run on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I spectre_amd/csrc
//       tools/poly_levels_check.cpp -o poly_levels_check
#include "poly_levels.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int fails = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAIL %s (n=%llu tile=%llu)\n", #c,               \
                        (unsigned long long)n, (unsigned long long)tile); \
            fails++;                                                      \
        }                                                                 \
    } while (0)

// marks [off, off + size) in `used`, which has `total` slots, for small cases
static void mark(std::vector<char>& used, uint64_t off, uint64_t size) {
    for (uint64_t i = 0; i < size; i++) used.at(off + i)++;
}

static void check(uint64_t n, uint64_t tile, uint32_t npoints) {
    // evaluation: down to one element, at least one level
    const PolyLevels ev = poly_levels(n, tile, 1, 1);
    CHECK(ev.ok && ev.count >= 1);
    uint64_t m = n, sum = 0;
    for (uint32_t l = 0; l < ev.count; l++) {
        CHECK(ev.size[l] == (m + tile - 1) / tile);
        CHECK(ev.off[l] == sum);
        sum += ev.size[l];
        m = ev.size[l];
    }
    CHECK(m == 1 && sum == ev.total);
    // division: until one tile remains, possibly no level at all
    const PolyLevels dv = poly_levels(n, tile, tile, 0);
    CHECK(dv.ok);
    m = n;
    sum = 0;
    for (uint32_t l = 0; l < dv.count; l++) {
        CHECK(m > tile);
        CHECK(dv.size[l] == (m + tile - 1) / tile);
        CHECK(dv.off[l] == sum);
        sum += dv.size[l];
        m = dv.size[l];
    }
    CHECK(m <= tile && sum == dv.total);
    if (ev.total * npoints > (1u << 22)) return;
    // the regions the host hands to the kernels: level l, point p at
    // npoints * off[l] + p * size[l]; the division adds one slot at the end
    std::vector<char> used(npoints * ev.total, 0);
    for (uint32_t l = 0; l < ev.count; l++)
        for (uint32_t p = 0; p < npoints; p++)
            mark(used, npoints * ev.off[l] + p * ev.size[l], ev.size[l]);
    for (char c : used) CHECK(c == 1);
    std::vector<char> used_dv(dv.total + 1, 0);
    for (uint32_t l = 0; l < dv.count; l++) mark(used_dv, dv.off[l], dv.size[l]);
    mark(used_dv, dv.total, 1);
    for (char c : used_dv) CHECK(c == 1);
}

int main() {
    const uint64_t kMaxN = 1ull << 28;
    for (uint64_t tile = 256; tile <= 1024; tile += 256) {
        std::vector<uint64_t> ns = {1, 2, 255, 256, 257, kMaxN - 1, kMaxN};
        for (uint64_t p = tile; p <= kMaxN; p *= tile)
            for (int d = -1; d <= 1; d++) ns.push_back(p + d);
        for (uint64_t p = 1; p <= kMaxN; p *= 2) ns.push_back(p + 1);
        for (uint64_t n : ns) {
            if (n == 0 || n > kMaxN) continue;
            // vectors per level: the points of fr_poly_eval, polynomials
            // times points (up to 32 * 8) in fr_poly_eval_batch
            for (uint32_t np : {1u, 3u, 8u, 15u, 256u}) check(n, tile, np);
        }
    }
    // a table that cannot hold the levels is reported, not overrun
    const uint64_t n = ~0ull, tile = 2;
    CHECK(!poly_levels(n, tile, 1, 1).ok);
    CHECK(!poly_levels(n, 1, 1, 1).ok);
    if (fails) std::printf("poly_levels_check: %d failures\n", fails);
    else std::printf("poly_levels_check: ok\n");
    return fails ? EXIT_FAILURE : EXIT_SUCCESS;
}
