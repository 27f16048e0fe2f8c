// poly_levels.hpp — index arithmetic of the opening-phase recursion in
// poly.hip (pure; host; no HIP, so a plain C++ program can check it under a
// sanitizer: tools/poly_levels_check.cpp).
#pragma once
#include <stdint.h>

// n <= 2^28 and tile >= 256 give at most 4 levels.
#define POLY_MAX_LEVELS 6

// The vectors of tile partials above an n-element vector, `tile` elements
// per tile: size[0] = ceil(n / tile), size[l] = ceil(size[l-1] / tile). A
// level is added while the vector below it has more than `stop` elements,
// and until there are `min_levels` of them. off[l] = elements of the levels
// before l, total = elements of all levels. ok = false (and nothing else
// valid) if the levels do not fit, which the callers' bound on n rules out.
struct PolyLevels {
    bool ok = true;
    uint32_t count = 0;
    uint64_t size[POLY_MAX_LEVELS] = {};
    uint64_t off[POLY_MAX_LEVELS] = {};
    uint64_t total = 0;
};

inline PolyLevels poly_levels(uint64_t n, uint64_t tile, uint64_t stop,
                              uint32_t min_levels) {
    PolyLevels lv;
    if (tile < 2 || stop < 1 || min_levels > POLY_MAX_LEVELS) {
        lv.ok = false;
        return lv;
    }
    uint64_t m = n;
    while (m > stop || lv.count < min_levels) {
        if (lv.count == POLY_MAX_LEVELS) {
            lv.ok = false;
            return lv;
        }
        m = m / tile + (m % tile != 0);
        lv.size[lv.count] = m;
        lv.off[lv.count] = lv.total;
        lv.total += m;
        lv.count++;
    }
    return lv;
}
