// poly.hip — Fr batch inversion and grand (running) products for gfx950.
//
// What halo2's permutation and lookup arguments do per Z column:
//   batch_invert(den); r = num * den^-1; Z[0] = z0, Z[i+1] = Z[i] * r[i]
// kept device-resident so the column never leaves the GPU between gate
// evaluation and its commit / transforms.
//
// Structure. A workgroup of POLY_THREADS threads owns one tile of
// POLY_THREADS * e consecutive elements, thread t the e consecutive elements
// [t*e, t*e + e) of it (e <= POLY_E_MAX is a launch argument; the loops are
// unrolled to POLY_E_MAX with wave-uniform guards, so the per-element arrays
// stay in registers for every e). Thread totals are combined through one
// binary product tree in LDS (heap order: node i has children 2i, 2i+1, the
// leaves are nodes POLY_THREADS.., the root is node 1):
//   up-sweep            node = left * right            -> root = tile product
//   down-sweep, invert  children <- (inv*right, inv*left): leaves end up
//                       holding the INVERSE of every thread total from one
//                       Fermat inversion of the root (Montgomery's trick run
//                       as a tree instead of a serial sweep)
//   down-sweep, scan    children <- (x, x*left): leaves end up holding the
//                       exclusive prefix of every thread, times the seed
// Field multiplication is exact and commutative, so the result bytes do not
// depend on the tile size or on the association order.
//
// Batch invert is one launch; no workgroup depends on another. The grand
// product is reduce-then-scan in three launches on the device's stream:
//   (A) k_gp_ratio   per tile: r = num * den^-1 -> d_z, tile product -> prods
//   (B) k_gp_prefix  ONE workgroup: prods -> exclusive prefixes seeded with
//                    z0, in tile-sized chunks with a carry; grand total last
//   (C) k_gp_scan    per tile: exclusive scan seeded with the tile's prefix
// There is no inter-workgroup waiting inside any kernel. Every thread reads
// all of its inputs before it writes its outputs and touches only its own
// indices, which is what lets d_out / d_z alias an input.
#include "internal.hpp"

#define POLY_THREADS 256
#define POLY_E_MAX 4  // elements per thread at the default tile
#define POLY_TILE_DEFAULT (POLY_THREADS * POLY_E_MAX)
#define POLY_MAX_N (1ull << 28)
// tree nodes 1 .. 2*POLY_THREADS-1, bank-split as in ntt.hip: the low 16 B of
// node i at lds4[i], the high 16 B at lds4[POLY_H + i] (lds_split_ld /
// lds_split_st), so consecutive nodes stride 4 banks instead of 8.
#define POLY_H (2 * POLY_THREADS)

// leaves <- v, then the up-sweep. On return (after its last barrier) node 1
// holds the product of all leaves. The leading barrier lets a caller reuse
// the tree right after reading from it.
__device__ __forceinline__ void tree_up(uint4* lds4, uint32_t t,
                                        const fp256& v) {
    __syncthreads();
    lds_split_st(lds4, POLY_THREADS + t, POLY_H, v);
    __syncthreads();
    for (uint32_t w = POLY_THREADS / 2; w >= 1; w >>= 1) {
        if (t < w) {
            fp256 a, b, c;
            lds_split_ld(lds4, 2 * (w + t), POLY_H, a);
            lds_split_ld(lds4, 2 * (w + t) + 1, POLY_H, b);
            ff_mul<Fr>(c, a, b);
            lds_split_st(lds4, w + t, POLY_H, c);
        }
        __syncthreads();
    }
}

// Down-sweep from node 1. kInvert: node 1 holds the inverse of the root
// product; every node is replaced by the inverse of its product. Otherwise:
// node 1 holds a seed; every node is replaced by seed * (product of all
// leaves left of its subtree). The caller reads leaf POLY_THREADS + t.
template <bool kInvert>
__device__ __forceinline__ void tree_down(uint4* lds4, uint32_t t) {
    for (uint32_t w = 1; w <= POLY_THREADS / 2; w <<= 1) {
        if (t < w) {
            const uint32_t i = w + t;
            fp256 x, l, r, o;
            lds_split_ld(lds4, i, POLY_H, x);
            lds_split_ld(lds4, 2 * i, POLY_H, l);
            if (kInvert) {
                lds_split_ld(lds4, 2 * i + 1, POLY_H, r);
                ff_mul<Fr>(o, x, r);
                lds_split_st(lds4, 2 * i, POLY_H, o);
            } else {
                lds_split_st(lds4, 2 * i, POLY_H, x);
            }
            ff_mul<Fr>(o, x, l);
            lds_split_st(lds4, 2 * i + 1, POLY_H, o);
        }
        __syncthreads();
    }
}

// x[k] = src[k] for k < e and k < cnt, else one. src points at the thread's
// first element, cnt = how many of its e elements exist (may be <= 0).
__device__ __forceinline__ void load_own(fp256 (&x)[POLY_E_MAX],
                                         const fp256* __restrict__ src,
                                         int64_t cnt, uint32_t e) {
#pragma unroll
    for (uint32_t k = 0; k < POLY_E_MAX; k++) {
        if (k < e && (int64_t)k < cnt) x[k] = src[k];
        else ff_set_one<Fr>(x[k]);
    }
}

// p[k] = x[0] * ... * x[k] for k < e (p[0] is x[0] itself); returns the
// thread total in tot.
__device__ __forceinline__ void own_prefixes(fp256 (&p)[POLY_E_MAX],
                                             fp256& tot,
                                             const fp256 (&x)[POLY_E_MAX],
                                             uint32_t e) {
    tot = x[0];
    p[0] = x[0];
#pragma unroll
    for (uint32_t k = 1; k < POLY_E_MAX; k++) {
        if (k < e) ff_mul<Fr>(tot, tot, x[k]);
        p[k] = tot;
    }
}

// In place: x[k] <- x[k]^-1 for k < e, zero staying zero. One Fermat
// inversion per workgroup (wave 0, every lane on the same value, so the wave
// never diverges).
__device__ __forceinline__ void tile_invert(uint4* lds4, uint32_t t,
                                            fp256 (&x)[POLY_E_MAX],
                                            uint32_t e) {
    uint32_t zmask = 0;
#pragma unroll
    for (uint32_t k = 0; k < POLY_E_MAX; k++) {
        if (ff_is_zero(x[k])) {
            zmask |= 1u << k;
            ff_set_one<Fr>(x[k]);
        }
    }
    fp256 p[POLY_E_MAX], inv;
    own_prefixes(p, inv, x, e);
    tree_up(lds4, t, inv);
    if (t < 64) {
        fp256 root, rinv;
        lds_split_ld(lds4, 1, POLY_H, root);
        ff_inv<Fr>(rinv, root);
        if (t == 0) lds_split_st(lds4, 1, POLY_H, rinv);
    }
    __syncthreads();
    tree_down<true>(lds4, t);
    lds_split_ld(lds4, POLY_THREADS + t, POLY_H, inv);  // (thread total)^-1
    // backward sweep: inv = (x[0] .. x[k])^-1 on entry to step k
#pragma unroll
    for (uint32_t k = POLY_E_MAX - 1; k >= 1; k--) {
        if (k < e) {
            fp256 o;
            ff_mul<Fr>(o, inv, p[k - 1]);
            ff_mul<Fr>(inv, inv, x[k]);
            x[k] = o;
        }
    }
    x[0] = inv;
#pragma unroll
    for (uint32_t k = 0; k < POLY_E_MAX; k++)
        if (zmask & (1u << k)) ff_set_zero(x[k]);
}

__global__ __launch_bounds__(POLY_THREADS) void k_fr_batch_invert(
    const fp256* in, fp256* out, uint64_t n, uint32_t e) {
    __shared__ uint4 lds4[2 * POLY_H];
    const uint32_t t = threadIdx.x;
    const uint64_t first = ((uint64_t)blockIdx.x * POLY_THREADS + t) * e;
    const int64_t cnt = (int64_t)n - (int64_t)first;
    fp256 x[POLY_E_MAX];
    load_own(x, in + first, cnt, e);
    tile_invert(lds4, t, x, e);
#pragma unroll
    for (uint32_t k = 0; k < POLY_E_MAX; k++)
        if (k < e && (int64_t)k < cnt) out[first + k] = x[k];
}

// (A) kDen: z = num * den^-1 and the tile's product of z -> prods[tile].
// !kDen: only the tile's product of num (the scan then reads num itself).
template <bool kDen>
__global__ __launch_bounds__(POLY_THREADS) void k_gp_ratio(
    const fp256* num, const fp256* den, fp256* z, fp256* __restrict__ prods,
    uint64_t n, uint32_t e) {
    __shared__ uint4 lds4[2 * POLY_H];
    const uint32_t t = threadIdx.x;
    const uint64_t first = ((uint64_t)blockIdx.x * POLY_THREADS + t) * e;
    const int64_t cnt = (int64_t)n - (int64_t)first;
    fp256 u[POLY_E_MAX];
    load_own(u, num + first, cnt, e);
    if (kDen) {
        fp256 d[POLY_E_MAX];
        load_own(d, den + first, cnt, e);
        tile_invert(lds4, t, d, e);
#pragma unroll
        for (uint32_t k = 0; k < POLY_E_MAX; k++) {
            if (k < e && (int64_t)k < cnt) {
                ff_mul<Fr>(u[k], u[k], d[k]);
                z[first + k] = u[k];
            }
        }
    }
    fp256 tot = u[0];
#pragma unroll
    for (uint32_t k = 1; k < POLY_E_MAX; k++)
        if (k < e) ff_mul<Fr>(tot, tot, u[k]);
    tree_up(lds4, t, tot);
    if (t == 0) {
        lds_split_ld(lds4, 1, POLY_H, tot);
        prods[blockIdx.x] = tot;
    }
}

// dst[i] = seed * src[0] * ... * src[i-1] for the cnt elements of one tile
// (src, dst point at the tile; they may be the same). Returns the product of
// the tile's elements to every thread.
__device__ __forceinline__ void tile_scan(uint4* lds4, uint32_t t,
                                          const fp256* src, fp256* dst,
                                          int64_t cnt, const fp256& seed,
                                          uint32_t e, fp256& total) {
    const uint64_t first = (uint64_t)t * e;
    const int64_t own = cnt - (int64_t)first;
    fp256 x[POLY_E_MAX], p[POLY_E_MAX], pre;
    load_own(x, src + first, own, e);
    own_prefixes(p, pre, x, e);
    tree_up(lds4, t, pre);
    lds_split_ld(lds4, 1, POLY_H, total);
    __syncthreads();
    if (t == 0) lds_split_st(lds4, 1, POLY_H, seed);
    __syncthreads();
    tree_down<false>(lds4, t);
    // seed * everything before x[0]
    lds_split_ld(lds4, POLY_THREADS + t, POLY_H, pre);
    if (own > 0) dst[first] = pre;
#pragma unroll
    for (uint32_t k = 1; k < POLY_E_MAX; k++) {
        if (k < e && (int64_t)k < own) {
            fp256 o;
            ff_mul<Fr>(o, pre, p[k - 1]);
            dst[first + k] = o;
        }
    }
}

// (B) one workgroup: prods[0..ntiles) -> exclusive prefixes seeded with z0,
// in place; prods[ntiles] = z0 * all of them.
__global__ __launch_bounds__(POLY_THREADS) void k_gp_prefix(
    fp256* prods, uint32_t ntiles, fp256 z0, uint32_t e) {
    __shared__ uint4 lds4[2 * POLY_H];
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = POLY_THREADS * e;
    fp256 carry = z0;
    for (uint32_t c0 = 0; c0 < ntiles; c0 += chunk) {
        fp256 total;
        tile_scan(lds4, t, prods + c0, prods + c0, (int64_t)ntiles - c0, carry,
                  e, total);
        ff_mul<Fr>(carry, carry, total);
    }
    if (t == 0) prods[ntiles] = carry;
}

// (C) per tile: exclusive scan of src seeded with the tile's prefix.
__global__ __launch_bounds__(POLY_THREADS) void k_gp_scan(
    const fp256* src, fp256* dst, const fp256* __restrict__ prefixes,
    uint64_t n, uint32_t e) {
    __shared__ uint4 lds4[2 * POLY_H];
    const uint64_t base = (uint64_t)blockIdx.x * POLY_THREADS * e;
    const fp256 seed = prefixes[blockIdx.x];
    fp256 total;
    tile_scan(lds4, threadIdx.x, src + base, dst + base,
              (int64_t)(n - base), seed, e, total);
}

// ---------------------------------------------------------------- host side
uint32_t fr_scan_tile_default() { return POLY_TILE_DEFAULT; }

bool fr_scan_tile_valid(uint32_t elems) {
    return elems == 0 ||
           (elems % POLY_THREADS == 0 && elems <= POLY_TILE_DEFAULT);
}

static uint32_t elems_per_thread(const spectre_gpu_ctx* ctx) {
    const uint32_t tile =
        ctx->fr_scan_tile ? ctx->fr_scan_tile : POLY_TILE_DEFAULT;
    return tile / POLY_THREADS;
}

int fr_batch_invert_device(spectre_gpu_ctx* ctx, int dev, const fp256* d_in,
                           fp256* d_out, uint64_t n) {
    if (n > POLY_MAX_N) {
        set_err("fr_batch_invert: n %llu > 2^28", (unsigned long long)n);
        return -1;
    }
    if (n == 0) return 0;
    DeviceState& ds = ctx->devs[dev];
    HIP_TRY(hipSetDevice(ds.device_id));
    const uint32_t e = elems_per_thread(ctx);
    const uint64_t tile = (uint64_t)POLY_THREADS * e;
    hipLaunchKernelGGL(k_fr_batch_invert, dim3((uint32_t)((n + tile - 1) / tile)),
                       dim3(POLY_THREADS), 0, ds.stream, d_in, d_out, n, e);
    HIP_TRY(hipStreamSynchronize(ds.stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

int fr_grand_product_device(spectre_gpu_ctx* ctx, int dev, const fp256* d_num,
                            const fp256* d_den, const fp256& z0, fp256* d_z,
                            uint64_t n, fp256* out_last) {
    if (n > POLY_MAX_N) {
        set_err("fr_grand_product: n %llu > 2^28", (unsigned long long)n);
        return -1;
    }
    if (n == 0) {
        if (out_last) *out_last = z0;
        return 0;
    }
    DeviceState& ds = ctx->devs[dev];
    HIP_TRY(hipSetDevice(ds.device_id));
    const uint32_t e = elems_per_thread(ctx);
    const uint64_t tile = (uint64_t)POLY_THREADS * e;
    const uint32_t ntiles = (uint32_t)((n + tile - 1) / tile);
    RC_TRY(ds.d_gp_prods.reserve((size_t)ntiles + 1));
    RC_TRY(ds.h_gp_last.reserve(1));
    fp256* prods = ds.d_gp_prods.ptr;
    if (d_den)
        hipLaunchKernelGGL(k_gp_ratio<true>, dim3(ntiles), dim3(POLY_THREADS),
                           0, ds.stream, d_num, d_den, d_z, prods, n, e);
    else
        hipLaunchKernelGGL(k_gp_ratio<false>, dim3(ntiles), dim3(POLY_THREADS),
                           0, ds.stream, d_num, d_den, d_z, prods, n, e);
    hipLaunchKernelGGL(k_gp_prefix, dim3(1), dim3(POLY_THREADS), 0, ds.stream,
                       prods, ntiles, z0, e);
    hipLaunchKernelGGL(k_gp_scan, dim3(ntiles), dim3(POLY_THREADS), 0,
                       ds.stream, d_den ? (const fp256*)d_z : d_num, d_z,
                       (const fp256*)prods, n, e);
    if (out_last)
        HIP_TRY(hipMemcpyAsync(ds.h_gp_last.ptr, prods + ntiles, sizeof(fp256),
                               hipMemcpyDeviceToHost, ds.stream));
    HIP_TRY(hipStreamSynchronize(ds.stream));
    HIP_TRY(hipGetLastError());
    if (out_last) *out_last = *ds.h_gp_last.ptr;
    return 0;
}
