// powtab.hip — the one builder of power tables (powtab.hpp).
//
// An entry g^e is a product of one constant per base-4 digit of e,
// c[w][d - 1] = g^(d * 4^w): the host squares its way up the 14 windows (a
// few dozen multiplies) and hands them over in the kernel arguments, so an
// entry costs at most 6 (T1) or 8 (T2) dependent multiplies where a
// square-and-multiply chain per entry costs up to 24 — the build is a
// latency chain on a handful of waves, and its depth is its time. T1's
// exponent j uses windows 0..5, T2's exponent 4096 j windows 6..13. Computes
// in FrCios whatever multiply the callers look up with: the bytes are the same.
#include "internal.hpp"

using PowFr = FrCios;

#define THREADS 256
#define POW_WINDOWS 14  // base-4 digits of an exponent < 2^28
struct PowWindows { fp256 c[POW_WINDOWS][3]; };
// dst[j] = scale * g^(j * 4^w0), j < count; nwin = base-4 digits of count - 1
struct PowRange {
    fp256* dst;
    uint32_t count, w0, nwin;
    fp256 scale;
};

// Blocks [0, nba) fill range a, the blocks from nba on range b.
__global__ __launch_bounds__(THREADS) void k_pow_tables(
    PowWindows pw, PowRange a, PowRange b, uint32_t nba) {
    const bool second = blockIdx.x >= nba;
    const PowRange& r = second ? b : a;
    const uint32_t j =
        (blockIdx.x - (second ? nba : 0u)) * blockDim.x + threadIdx.x;
    if (j >= r.count) return;
    fp256 acc = r.scale;
#pragma unroll 1
    for (uint32_t w = 0; w < r.nwin; w++) {
        const uint32_t d = (j >> (2 * w)) & 3u;
        fp256 f, t;
#pragma unroll
        for (int i = 0; i < 8; i++)
            f.l[i] = d == 1 ? pw.c[r.w0 + w][0].l[i]
                            : (d == 2 ? pw.c[r.w0 + w][1].l[i]
                                      : pw.c[r.w0 + w][2].l[i]);
        ff_mul<PowFr>(t, acc, f);
#pragma unroll
        for (int i = 0; i < 8; i++) acc.l[i] = d ? t.l[i] : acc.l[i];
    }
    r.dst[j] = acc;
}

// count >= 1, w0 + nwin <= POW_WINDOWS; a null scale is 1
static PowRange pow_range(fp256* dst, uint32_t count, uint32_t w0,
                          const fp256* scale) {
    PowRange r{dst, count, w0, 0, {}};
    for (uint32_t x = count - 1; x; x >>= 2) r.nwin++;
    if (scale) r.scale = *scale;
    else ff_set_one<PowFr>(r.scale);
    return r;
}

// one launch for a and, where b.count != 0, b
static void pow_launch(DeviceState& ds, const fp256& g, const PowRange& a,
                       const PowRange& b) {
    PowWindows pw;
    fp256 x = g;
    for (int w = 0; w < POW_WINDOWS; w++) {
        pw.c[w][0] = x;
        ff_sqr<PowFr>(pw.c[w][1], x);
        ff_mul<PowFr>(pw.c[w][2], pw.c[w][1], x);
        ff_sqr<PowFr>(x, pw.c[w][1]);
    }
    const uint32_t nba = (a.count + THREADS - 1) / THREADS;
    const uint32_t nbb = (b.count + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(k_pow_tables, dim3(nba + nbb), dim3(THREADS), 0,
                       ds.stream, pw, a, b, nba);
}

PowTable pow_tables_build(DeviceState& ds, const fp256& g, const fp256* scale,
                          uint64_t n, fp256* dst) {
    const uint32_t t1n = n < POW_LOW ? (uint32_t)n : POW_LOW;
    const uint32_t t2n = (uint32_t)(pow_table_elems(n) - POW_LOW);
    pow_launch(ds, g, pow_range(dst, t1n, 0, nullptr),
               pow_range(dst + POW_LOW, t2n, POW_LOW_BITS / 2, scale));
    return PowTable{dst, dst + POW_LOW};
}

void pow_linear_build(DeviceState& ds, const fp256& g, fp256* out,
                      uint32_t count) {
    pow_launch(ds, g, pow_range(out, count, 0, nullptr), PowRange{});
}
