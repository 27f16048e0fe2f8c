// poly.hip — Fr batch inversion and grand (running) products, and the opening
// phase's polynomial evaluation and (X - z) division, for gfx950.
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
//
// Opening phase: eval_polynomial and kate_division on the same tiles, with
// zero for padding and a second, ADDITIVE tree with weights. For a point x a
// thread forms S = sum_k a[f+k] x^k over its e coefficients by Horner from
// the top, and the up-sweep combines
//   node = left + x^(len_left) * right               -> root = tile partial
// with the eight weights x^(e*2^l) taken from a host-built table in the
// kernel arguments. The tile partials P_b = sum_k a[bT+k] x^k are a
// polynomial P with a(x) = P(x^T), so
//   evaluation  is k_poly_tile_eval run to a fixed point: the host loops
//               n -> ceil(n/T) -> .. -> 1, raising the point to the T-th
//               power per level; there is no separate final reduction. For
//               several points a thread keeps its coefficients in registers
//               and loops the points (one read of a); above the first level
//               each point has its own vector, on gridDim.y.
//   division    a(X) = (X - z) q(X) + rem is reduce-then-scan over the same
//               partials from the top index down. With Q[i] the quotient at
//               index i, the seed of tile b is Q[(b+1)T - 1] = C_b where
//               C = div(P, z^T): the same problem one level up. The host
//               evaluates partials level by level until one tile remains,
//               divides that tile with seed 0 (its root is rem = a(z)), and
//               descends with one k_poly_div_scan per level, each tile seeded
//               from the level above; partial vectors become their quotients
//               in place. In a tile the down-sweep hands a node's seed to its
//               right child and S_right + z^(len_right) * seed to its left
//               child; thread t then has q[f+e-1] = seed_t and
//               q[k] = a[k+1] + z q[k+1] down to k = f.
// No inverse of z is taken, so z = 0 and z = 1 are ordinary inputs. Field
// addition and multiplication are exact, so here too the result bytes depend
// neither on the tile size nor on the association order. A thread reads all
// of a[f, f+e) before it writes q[f, f+e) and touches no other index of
// either, which is what lets d_q alias d_a.
//
// Set-level forms (multiopen). fr_poly_eval_batch is the evaluation above
// with a third grid dimension: z is the polynomial, taken at the first level
// from a pointer table in the kernel arguments, and every level runs the
// partial vectors of all m polynomials and all points in one launch, so the
// launches per call do not grow with m and one readback returns m * npoints
// values. fr_poly_div_roots enqueues the division above once per root, the
// first from d_a and the rest in place in d_q, and synchronizes once.
#include "internal.hpp"
#include "poly_levels.hpp"

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

// ------------------------------------------------------------ opening phase
#define POLY_TREE_LEVELS 8  // log2(POLY_THREADS)
static_assert(1u << POLY_TREE_LEVELS == POLY_THREADS, "one weight per level");
// Powers of one point for a launch with e elements per thread, built on the
// host: w[0] = x, w[1 + l] = x^(e * 2^l), the weight of a right child whose
// left sibling spans 2^l threads.
struct PolyPow {
    fp256 w[1 + POLY_TREE_LEVELS];
};
struct PolyPows {
    PolyPow pt[SPECTRE_POLY_EVAL_MAX_POINTS];
};

// x[k] = src[k] for k < e and k < cnt, else zero (load_own with the additive
// identity).
__device__ __forceinline__ void load_own_zero(fp256 (&x)[POLY_E_MAX],
                                              const fp256* src, int64_t cnt,
                                              uint32_t e) {
#pragma unroll
    for (uint32_t k = 0; k < POLY_E_MAX; k++) {
        if (k < e && (int64_t)k < cnt) x[k] = src[k];
        else ff_set_zero(x[k]);
    }
}

// s = sum_{k<e} a[k] x^k by Horner from the top (a[k] = 0 for k >= e).
__device__ __forceinline__ void own_horner(fp256& s,
                                           const fp256 (&a)[POLY_E_MAX],
                                           const fp256& x, uint32_t e) {
    s = a[POLY_E_MAX - 1];
#pragma unroll
    for (int k = POLY_E_MAX - 2; k >= 0; k--) {
        if ((uint32_t)k + 1 < e) ff_mul<Fr>(s, s, x);
        ff_add<Fr>(s, s, a[k]);
    }
}

// leaves <- v, then the weighted additive up-sweep: node = left + w * right,
// w = pw.w[1 + l] at the level whose children span 2^l threads. On return
// every node holds the Horner value of its subtree, node 1 the tile's. Same
// barriers as tree_up.
__device__ __forceinline__ void wtree_up(uint4* lds4, uint32_t t,
                                         const fp256& v, const PolyPow& pw) {
    __syncthreads();
    lds_split_st(lds4, POLY_THREADS + t, POLY_H, v);
    __syncthreads();
    uint32_t l = 0;
    for (uint32_t w = POLY_THREADS / 2; w >= 1; w >>= 1, l++) {
        if (t < w) {
            fp256 a, b, c;
            lds_split_ld(lds4, 2 * (w + t), POLY_H, a);
            lds_split_ld(lds4, 2 * (w + t) + 1, POLY_H, b);
            ff_mul<Fr>(c, b, pw.w[1 + l]);
            ff_add<Fr>(c, c, a);
            lds_split_st(lds4, w + t, POLY_H, c);
        }
        __syncthreads();
    }
}

// Down-sweep of the division after wtree_up, node 1 holding the tile's seed
// (the quotient value just above the tile): a node's seed goes to its right
// child, and S_right + w * seed to its left child, w = z^(len_right). Leaf
// POLY_THREADS + t ends up holding the quotient value just above thread t's
// elements.
__device__ __forceinline__ void wtree_down(uint4* lds4, uint32_t t,
                                           const PolyPow& pw) {
    uint32_t l = POLY_TREE_LEVELS;
    for (uint32_t w = 1; w <= POLY_THREADS / 2; w <<= 1) {
        l--;
        if (t < w) {
            const uint32_t i = w + t;
            fp256 x, r, o;
            lds_split_ld(lds4, i, POLY_H, x);
            lds_split_ld(lds4, 2 * i + 1, POLY_H, r);
            ff_mul<Fr>(o, x, pw.w[1 + l]);
            ff_add<Fr>(o, o, r);
            lds_split_st(lds4, 2 * i, POLY_H, o);
            lds_split_st(lds4, 2 * i + 1, POLY_H, x);
        }
        __syncthreads();
    }
}

// Tile partials. Block (b, y, z) works for polynomial z of a batch (one, z =
// 0, outside fr_poly_eval_batch) and the ppb points p = y * ppb + j of the
// call's npts = gridDim.y * ppb: it reads tile b of its n-element vector src
// once and, for each p, writes sum_k src[bT + k] x_p^k to row z * npts + p of
// partials, at column b. The POINT table is indexed by p alone, the partial
// VECTOR by (z, p).
__device__ __forceinline__ void poly_tile_eval(
    uint4* lds4, const fp256* __restrict__ src, uint64_t n,
    fp256* __restrict__ partials, uint64_t part_stride, uint32_t ppb,
    uint32_t e, const PolyPows& pws) {
    const uint32_t t = threadIdx.x;
    const uint64_t first = ((uint64_t)blockIdx.x * POLY_THREADS + t) * e;
    const int64_t cnt = (int64_t)n - (int64_t)first;
    const uint32_t row0 = blockIdx.z * gridDim.y * ppb;
    fp256 a[POLY_E_MAX];
    load_own_zero(a, src + first, cnt, e);
    for (uint32_t j = 0; j < ppb; j++) {
        const uint32_t p = blockIdx.y * ppb + j;
        const PolyPow& pw = pws.pt[p];
        fp256 s;
        own_horner(s, a, pw.w[0], e);
        wtree_up(lds4, t, s, pw);
        if (t == 0) {
            lds_split_ld(lds4, 1, POLY_H, s);
            partials[(uint64_t)(row0 + p) * part_stride + blockIdx.x] = s;
        }
    }
}

// The vectors lie src_stride apart, one per (z, y): the first level of
// fr_poly_eval runs one y with all the points (one read of the
// coefficients); the levels above it, in the batch too, one point per y, each
// on the partial vector of its own (z, p).
__global__ __launch_bounds__(POLY_THREADS) void k_poly_tile_eval(
    const fp256* __restrict__ src, uint64_t src_stride, uint64_t n,
    fp256* __restrict__ partials, uint64_t part_stride, uint32_t ppb,
    uint32_t e, const PolyPows pws) {
    __shared__ uint4 lds4[2 * POLY_H];
    const uint64_t vec = (uint64_t)blockIdx.z * gridDim.y + blockIdx.y;
    poly_tile_eval(lds4, src + vec * src_stride, n, partials, part_stride, ppb,
                   e, pws);
}

// The first level of a batch: polynomial z comes from a pointer table in the
// kernel arguments (32 * 8 B beside the 2304 B of powers), one y, all the
// points.
struct PolyPtrs {
    const fp256* p[SPECTRE_OPEN_MAX_POLYS];
};
__global__ __launch_bounds__(POLY_THREADS) void k_poly_tile_eval_tab(
    const PolyPtrs tab, uint64_t n, fp256* __restrict__ partials,
    uint64_t part_stride, uint32_t ppb, uint32_t e, const PolyPows pws) {
    __shared__ uint4 lds4[2 * POLY_H];
    poly_tile_eval(lds4, tab.p[blockIdx.z], n, partials, part_stride, ppb, e,
                   pws);
}

// One level of the division: dst[i] = the quotient of the n-element vector
// src by (X - z) at index i, given seeds[b] = the quotient value just above
// tile b (null: zero, the top level). src and dst may be the same. rem_out
// (null below the top level, where there is one tile) receives the tile's
// Horner value, which at the top is a(z).
__global__ __launch_bounds__(POLY_THREADS) void k_poly_div_scan(
    const fp256* src, fp256* dst, const fp256* __restrict__ seeds, uint64_t n,
    fp256* __restrict__ rem_out, uint32_t e, const PolyPow pw) {
    __shared__ uint4 lds4[2 * POLY_H];
    const uint32_t t = threadIdx.x;
    const uint64_t first = ((uint64_t)blockIdx.x * POLY_THREADS + t) * e;
    const int64_t cnt = (int64_t)n - (int64_t)first;
    fp256 a[POLY_E_MAX], q;
    load_own_zero(a, src + first, cnt, e);
    own_horner(q, a, pw.w[0], e);
    wtree_up(lds4, t, q, pw);
    if (t == 0) {
        if (rem_out) {
            lds_split_ld(lds4, 1, POLY_H, q);
            *rem_out = q;
        }
        if (seeds) q = seeds[blockIdx.x];
        else ff_set_zero(q);
        lds_split_st(lds4, 1, POLY_H, q);
    }
    __syncthreads();
    wtree_down(lds4, t, pw);
    lds_split_ld(lds4, POLY_THREADS + t, POLY_H, q);  // q[first + e - 1]
    // the guards are wave-uniform in k and e; a[k] beyond e or n is zero
#pragma unroll
    for (int k = POLY_E_MAX - 1; k >= 0; k--) {
        if ((uint32_t)k < e) {
            if ((int64_t)k < cnt) dst[first + k] = q;
            if (k > 0) {
                ff_mul<Fr>(q, q, pw.w[0]);
                ff_add<Fr>(q, q, a[k]);
            }
        }
    }
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
    return call_finish(ds);
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
    // tile products -> prefixes, the grand total last
    RC_TRY(ds.d_call.reserve(((size_t)ntiles + 1) * sizeof(fp256)));
    fp256* prods = (fp256*)ds.d_call.ptr;
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
    return call_finish(ds, out_last, prods + ntiles, sizeof(fp256));
}

// The table of x for a launch with e elements per thread; returns x^(256 e),
// the point of the level above.
static fp256 poly_pow_table(PolyPow& pw, const fp256& x, uint32_t e) {
    pw.w[0] = x;
    ff_pow_u32<Fr>(pw.w[1], x, e);
    for (int l = 1; l < POLY_TREE_LEVELS; l++)
        ff_sqr<Fr>(pw.w[1 + l], pw.w[l]);
    fp256 up;
    ff_sqr<Fr>(up, pw.w[POLY_TREE_LEVELS]);
    return up;
}

static uint32_t poly_tiles(uint64_t n, uint64_t tile) {
    return (uint32_t)((n + tile - 1) / tile);
}

// out[k * npoints + p] = polynomial k at point p, for the one polynomial
// d_coeffs (npolys = 1) or, d_coeffs null, the npolys of d_polys.
static int poly_eval_run(spectre_gpu_ctx* ctx, int dev, const char* what,
                         const fp256* d_coeffs, const fp256* const* d_polys,
                         uint32_t npolys, uint64_t n, const fp256* points,
                         uint32_t npoints, fp256* out) {
    const uint32_t nvec = npolys * npoints;
    if (n > POLY_MAX_N) {
        set_err("%s: n %llu > 2^28", what, (unsigned long long)n);
        return -1;
    }
    if (n == 0) {
        for (uint32_t v = 0; v < nvec; v++) ff_set_zero(out[v]);
        return 0;
    }
    DeviceState& ds = ctx->devs[dev];
    HIP_TRY(hipSetDevice(ds.device_id));
    const uint32_t e = elems_per_thread(ctx);
    const uint64_t tile = (uint64_t)POLY_THREADS * e;
    // partial vectors down to one element per polynomial and point; level l
    // holds nvec vectors of size[l] from element nvec * off[l], polynomial
    // k's at point p being number k * npoints + p
    const PolyLevels lv = poly_levels(n, tile, 1, 1);
    if (!lv.ok) {
        set_err("%s: level table overflow at n %llu", what,
                (unsigned long long)n);
        return -1;
    }
    RC_TRY(ds.d_call.reserve(nvec * lv.total * sizeof(fp256)));
    fp256* const parts = (fp256*)ds.d_call.ptr;
    fp256 x[SPECTRE_POLY_EVAL_MAX_POINTS];
    for (uint32_t p = 0; p < npoints; p++) x[p] = points[p];
    const fp256* src = d_coeffs;
    uint64_t m = n;
    for (uint32_t l = 0; l < lv.count; l++) {
        PolyPows pws{};
        for (uint32_t p = 0; p < npoints; p++)
            x[p] = poly_pow_table(pws.pt[p], x[p], e);
        fp256* dst = parts + nvec * lv.off[l];
        // the coefficients serve every point; above them, a vector per point
        const uint32_t ny = l == 0 ? 1 : npoints;
        const dim3 grid(poly_tiles(m, tile), ny, npolys);
        if (l == 0 && !d_coeffs) {
            PolyPtrs tab{};
            for (uint32_t k = 0; k < npolys; k++) tab.p[k] = d_polys[k];
            hipLaunchKernelGGL(k_poly_tile_eval_tab, grid, dim3(POLY_THREADS),
                               0, ds.stream, tab, m, dst, lv.size[l],
                               npoints / ny, e, pws);
        } else {
            hipLaunchKernelGGL(k_poly_tile_eval, grid, dim3(POLY_THREADS), 0,
                               ds.stream, src, m, m, dst, lv.size[l],
                               npoints / ny, e, pws);
        }
        src = dst;
        m = lv.size[l];
    }
    // the last level is one element per polynomial and point, contiguous
    return call_finish(ds, out, src, nvec * sizeof(fp256));
}

int fr_poly_eval_device(spectre_gpu_ctx* ctx, int dev, const fp256* d_coeffs,
                        uint64_t n, const fp256* points, uint32_t npoints,
                        fp256* out) {
    return poly_eval_run(ctx, dev, "fr_poly_eval", d_coeffs, nullptr, 1, n,
                         points, npoints, out);
}

int fr_poly_eval_batch_device(spectre_gpu_ctx* ctx, int dev,
                              const fp256* const* d_polys, uint32_t npolys,
                              uint64_t n, const fp256* points,
                              uint32_t npoints, fp256* out) {
    return poly_eval_run(ctx, dev, "fr_poly_eval_batch", nullptr, d_polys,
                         npolys, n, points, npoints, out);
}

// Enqueues one division of the n elements at d_a by (X - z) into d_q (which
// may be d_a), the remainder into *d_rem; parts = lv.total elements of the
// arena, free again once the launches have run.
static void poly_div_enqueue(DeviceState& ds, uint32_t e, const PolyLevels& lv,
                             fp256* parts, fp256* d_rem, const fp256* d_a,
                             const fp256& z, fp256* d_q, uint64_t n) {
    const uint64_t tile = (uint64_t)POLY_THREADS * e;
    // vec[0] = a, vec[l] = the partials of vec[l - 1], at the point zl[l]
    const fp256* vec[POLY_MAX_LEVELS + 1];
    uint64_t len[POLY_MAX_LEVELS + 1];
    PolyPow zl[POLY_MAX_LEVELS + 1];
    vec[0] = d_a;
    len[0] = n;
    fp256 x = z;
    for (uint32_t l = 0; l <= lv.count; l++) {
        x = poly_pow_table(zl[l], x, e);
        if (l == lv.count) break;
        vec[l + 1] = parts + lv.off[l];
        len[l + 1] = lv.size[l];
        PolyPows one{};
        one.pt[0] = zl[l];
        hipLaunchKernelGGL(k_poly_tile_eval, dim3(poly_tiles(len[l], tile), 1),
                           dim3(POLY_THREADS), 0, ds.stream, vec[l], len[l],
                           len[l], parts + lv.off[l], lv.size[l], 1u, e, one);
    }
    for (int l = (int)lv.count; l >= 0; l--) {
        const bool top = l == (int)lv.count;
        hipLaunchKernelGGL(k_poly_div_scan, dim3(poly_tiles(len[l], tile)),
                           dim3(POLY_THREADS), 0, ds.stream, vec[l],
                           l == 0 ? d_q : parts + lv.off[l - 1],
                           top ? (const fp256*)nullptr : vec[l + 1], len[l],
                           top ? d_rem : (fp256*)nullptr, e, zl[l]);
    }
}

// nroots divisions in a row, the first d_a -> d_q and the rest in place in
// d_q, sharing the partial vectors (the stream runs them in order) and each
// with a remainder slot of its own; out_rems (may be null) = nroots elements.
static int poly_div_run(spectre_gpu_ctx* ctx, int dev, const char* what,
                        const fp256* d_a, const fp256* roots, uint32_t nroots,
                        fp256* d_q, uint64_t n, fp256* out_rems) {
    if (n > POLY_MAX_N) {
        set_err("%s: n %llu > 2^28", what, (unsigned long long)n);
        return -1;
    }
    if (n == 0) {
        for (uint32_t j = 0; out_rems && j < nroots; j++)
            ff_set_zero(out_rems[j]);
        return 0;
    }
    DeviceState& ds = ctx->devs[dev];
    HIP_TRY(hipSetDevice(ds.device_id));
    const uint32_t e = elems_per_thread(ctx);
    const uint64_t tile = (uint64_t)POLY_THREADS * e;
    // partial vectors until one fits a tile; one more element per a(z)
    const PolyLevels lv = poly_levels(n, tile, tile, 0);
    if (!lv.ok) {
        set_err("%s: level table overflow at n %llu", what,
                (unsigned long long)n);
        return -1;
    }
    RC_TRY(ds.d_call.reserve((lv.total + nroots) * sizeof(fp256)));
    fp256* parts = (fp256*)ds.d_call.ptr;
    fp256* d_rems = parts + lv.total;
    for (uint32_t j = 0; j < nroots; j++)
        poly_div_enqueue(ds, e, lv, parts, d_rems + j, j == 0 ? d_a : d_q,
                         roots[j], d_q, n);
    return call_finish(ds, out_rems, d_rems, nroots * sizeof(fp256));
}

int fr_poly_div_linear_device(spectre_gpu_ctx* ctx, int dev, const fp256* d_a,
                              const fp256& z, fp256* d_q, uint64_t n,
                              fp256* out_rem) {
    return poly_div_run(ctx, dev, "fr_poly_div_linear", d_a, &z, 1, d_q, n,
                        out_rem);
}

int fr_poly_div_roots_device(spectre_gpu_ctx* ctx, int dev, const fp256* d_a,
                             const fp256* roots, uint32_t nroots, fp256* d_q,
                             uint64_t n, fp256* out_rems) {
    return poly_div_run(ctx, dev, "fr_poly_div_roots", d_a, roots, nroots, d_q,
                        n, out_rems);
}
