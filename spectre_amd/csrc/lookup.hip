// lookup.hip — halo2's permute_expression_pair on the device, for gfx950.
//
// Per lookup argument halo2 turns the compressed input column A and table
// column S (u usable rows each) into
//   A' = A sorted ascending by canonical value (Fr::cmp), and
//   S' = S rearranged so that every row has A'[i] == S'[i] or
//        A'[i] == A'[i-1],
// with a sort and a serial walk over an ordered map: the first row of every
// run of equal values in A' takes its own value out of the table, and the
// table values left over fill the remaining ("repeated") rows, the smallest
// value going to the LAST repeated row. The same S', without the walk:
//   Ss = sort(S);  first[i] = (i == 0 || A'[i] != A'[i-1])
//   every first row marks taken[p], p = the lower bound of its value in Ss
//     (p == u or Ss[p] != A'[i]: the value is not in the table, a miss)
//   left = Ss without the taken entries, rep = the rows that are not first,
//     both ascending and both m long
//   S'[i] = A'[i] on first rows, S'[rep[k]] = left[m-1-k] on the others
// Distinct values have distinct lower bounds, so the marks never collide,
// and the two compactions are exclusive prefix sums.
//
// Launches, all on the device's stream, ordered by launch boundaries alone
// (no flags, spins or inter-workgroup waits inside a kernel):
//   k_lk_canon      both columns -> canonical scratch copies; every block
//                   ORs the canonical limbs it saw into eight words
//   (host)          reads the 32-byte OR: which 64-bit limbs hold any bit,
//                   and the highest bit of each
//   per column, per 64-bit limb that is not zero everywhere, low to high:
//     k_lk_limb_keys  key[i] = canon[perm[i]].limb
//     hipcub SortPairs (stable) on (key, perm), up to the limb's highest bit
//   k_lk_gather     A' (Montgomery, via the permutation) -> d_input_perm;
//                   Ss -> scratch, Montgomery and canonical
//   k_lk_search     first[], and on first rows the lower bound in canonical
//                   Ss: clears free[p] or counts a miss
//   (host)          reads the miss count; nonzero ends the call
//   hipcub ExclusiveSum of !first and of free
//   k_lk_first_rows S'[i] = A'[i] on first rows, rep[rank] = i on the others
//   k_lk_fill       S'[rep[m-1-k]] = left[k]
// Every row of S' is written exactly once, by one of the last two kernels.
// Skipping zero limbs and bits cannot change the result: a stable sort on a
// key that is equal everywhere is the identity.
//
// Elements move as two 16-byte halves per lane. The canonical value is only
// ever a sort and search key; every output byte is copied from an input.
#include "internal.hpp"
#include <hipcub/hipcub.hpp>

#define LK_THREADS 256
#define LK_CANON_MAX_BLOCKS 2048  // k_lk_canon strides; one OR per block
#define LK_WORDS 9                // 8 OR words, then the miss count
#define LK_MISS 8

// hipCUB reports a failed launch or a short temp buffer only through its
// return value; an unchecked one is a silently skipped sort.
#define CUB_TRY(x)                                                        \
    do {                                                                  \
        hipError_t _e = (x);                                              \
        if (_e != hipSuccess) {                                           \
            set_err("%s:%d %s: %s", __FILE__, __LINE__, #x,               \
                    hipGetErrorString(_e));                               \
            return -2;                                                    \
        }                                                                 \
    } while (0)

__device__ __forceinline__ void ld_halves(fp256& o, const fp256* p) {
    const uint4* q = (const uint4*)p;
    const uint4 lo = q[0], hi = q[1];
    memcpy(&o.l[0], &lo, 16);
    memcpy(&o.l[4], &hi, 16);
}
__device__ __forceinline__ void st_halves(fp256* p, const fp256& v) {
    uint4 lo, hi;
    memcpy(&lo, &v.l[0], 16);
    memcpy(&hi, &v.l[4], 16);
    uint4* q = (uint4*)p;
    q[0] = lo;
    q[1] = hi;
}

// a < b as 256-bit integers, from the top limb
__device__ __forceinline__ bool lk_less(const fp256& a, const fp256& b) {
    bool lt = false;
#pragma unroll
    for (int i = 0; i < 8; i++)  // a higher limb that differs overrides
        lt = a.l[i] != b.l[i] ? a.l[i] < b.l[i] : lt;
    return lt;
}

// canon[0, u) = canonical a, canon[u, 2u) = canonical s; or_words[0..8) |=
// every canonical limb (zeroed by the host before the launch).
__global__ __launch_bounds__(LK_THREADS) void k_lk_canon(
    const fp256* __restrict__ a, const fp256* __restrict__ s,
    fp256* __restrict__ canon, uint32_t u, uint32_t* __restrict__ or_words) {
    __shared__ uint32_t wave_or[LK_THREADS / 64][8];
    uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t total = 2 * u, stride = gridDim.x * LK_THREADS;
    for (uint32_t i = blockIdx.x * LK_THREADS + threadIdx.x; i < total;
         i += stride) {
        fp256 x, c;
        ld_halves(x, i < u ? a + i : s + (i - u));
        ff_from_mont<Fr>(c, x);
        st_halves(canon + i, c);
#pragma unroll
        for (int k = 0; k < 8; k++) acc[k] |= c.l[k];
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
            acc[k] |= __shfl_xor(acc[k], off);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) wave_or[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < LK_THREADS / 64; w++) v |= wave_or[w][threadIdx.x];
        if (v) atomicOr(&or_words[threadIdx.x], v);
    }
}

// keys[i] = 64-bit limb `limb` of canon[perm[i]]. kFirst: the pass that
// starts a column's sort; perm is the identity and is written here.
template <bool kFirst>
__global__ __launch_bounds__(LK_THREADS) void k_lk_limb_keys(
    const uint64_t* __restrict__ canon64, uint32_t limb, uint32_t* perm,
    uint64_t* __restrict__ keys, uint32_t u) {
    const uint32_t i = blockIdx.x * LK_THREADS + threadIdx.x;
    if (i >= u) return;
    uint32_t src = i;
    if (kFirst) perm[i] = i;
    else src = perm[i];
    keys[i] = canon64[4 * (size_t)src + limb];
}

// dst_mont[i] = src_mont[perm[i]]; kCanon: dst_canon[i] = src_canon[perm[i]].
template <bool kCanon>
__global__ __launch_bounds__(LK_THREADS) void k_lk_gather(
    const fp256* __restrict__ src_mont, const fp256* __restrict__ src_canon,
    const uint32_t* __restrict__ perm, fp256* __restrict__ dst_mont,
    fp256* __restrict__ dst_canon, uint32_t u) {
    const uint32_t i = blockIdx.x * LK_THREADS + threadIdx.x;
    if (i >= u) return;
    const uint32_t src = perm[i];
    fp256 x;
    ld_halves(x, src_mont + src);
    st_halves(dst_mont + i, x);
    if (kCanon) {
        ld_halves(x, src_canon + src);
        st_halves(dst_canon + i, x);
    }
}

// notfirst[i] = (A'[i] == A'[i-1]); a first row finds the lower bound p of
// its value in ss_canon and clears free_[p] (preset to one), or counts a
// miss. Equal reduced residues have equal bytes, so runs are found on the
// Montgomery image; only first rows pay for the canonical value.
__global__ __launch_bounds__(LK_THREADS) void k_lk_search(
    const fp256* __restrict__ a_perm, const fp256* __restrict__ ss_canon,
    uint32_t u, uint32_t* __restrict__ notfirst, uint32_t* __restrict__ free_,
    uint32_t* __restrict__ miss) {
    const uint32_t i = blockIdx.x * LK_THREADS + threadIdx.x;
    if (i >= u) return;
    fp256 x, prev;
    ld_halves(x, a_perm + i);
    bool first = true;
    if (i > 0) {
        ld_halves(prev, a_perm + (i - 1));
        first = !ff_eq(x, prev);
    }
    notfirst[i] = first ? 0u : 1u;
    if (!first) return;
    fp256 v, probe;
    ff_from_mont<Fr>(v, x);
    uint32_t lo = 0, hi = u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        ld_halves(probe, ss_canon + mid);
        if (lk_less(probe, v)) lo = mid + 1;
        else hi = mid;
    }
    bool hit = false;
    if (lo < u) {
        ld_halves(probe, ss_canon + lo);
        hit = ff_eq(probe, v);
    }
    if (hit) free_[lo] = 0u;
    else atomicAdd(miss, 1u);
}

// First rows take their own value; the others queue up in rep, ascending.
__global__ __launch_bounds__(LK_THREADS) void k_lk_first_rows(
    const fp256* __restrict__ a_perm, fp256* __restrict__ s_perm,
    const uint32_t* __restrict__ notfirst,
    const uint32_t* __restrict__ rank_rep, uint32_t* __restrict__ rep,
    uint32_t u) {
    const uint32_t i = blockIdx.x * LK_THREADS + threadIdx.x;
    if (i >= u) return;
    if (notfirst[i]) {
        rep[rank_rep[i]] = i;
    } else {
        fp256 x;
        ld_halves(x, a_perm + i);
        st_halves(s_perm + i, x);
    }
}

// The k-th table value left over goes to the k-th repeated row from the end.
// m = the number of repeated rows, from the last flag and its rank; a call
// without a miss has exactly as many values left.
__global__ __launch_bounds__(LK_THREADS) void k_lk_fill(
    const fp256* __restrict__ ss_mont, const uint32_t* __restrict__ free_,
    const uint32_t* __restrict__ rank_left,
    const uint32_t* __restrict__ notfirst,
    const uint32_t* __restrict__ rank_rep, const uint32_t* __restrict__ rep,
    fp256* __restrict__ s_perm, uint32_t u) {
    const uint32_t j = blockIdx.x * LK_THREADS + threadIdx.x;
    if (j >= u || !free_[j]) return;
    const uint32_t m = rank_rep[u - 1] + notfirst[u - 1];
    const uint32_t k = rank_left[j];
    if (k >= m) return;
    fp256 x;
    ld_halves(x, ss_mont + j);
    st_halves(s_perm + rep[m - 1 - k], x);
}

// ---------------------------------------------------------------- host side
static uint32_t lk_blocks(uint32_t n) {
    return (n + LK_THREADS - 1) / LK_THREADS;
}

// Scratch of one call over u rows, carved out of the call arena.
struct LkScratch {
    fp256* canon;     // 2u: canonical input (later canonical Ss) | table
    fp256* ss;        // u: the sorted table, Montgomery
    uint64_t* keys;   // 2u: one limb's sort keys, in | out
    uint32_t* idx;    // 7u: 2 permutations, !first, free, their ranks, rep
    uint32_t* words;  // LK_WORDS: OR of the canonical limbs, miss count
    uint8_t* tmp;     // hipCUB sort / scan temp storage
    size_t tmp_bytes;
};

// The temp sizes come from null typed pointers: rocPRIM returns the size
// before it looks at a key or value pointer.
static int lk_reserve(DeviceState& ds, uint32_t u, LkScratch& s) {
    size_t sort_need = 0, scan_need = 0;
    uint64_t* const k = nullptr;
    uint32_t* const x = nullptr;
    CUB_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_need, k, k, x, x,
                                               (int64_t)u, 0, 64, ds.stream));
    CUB_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_need, x, x, (int)u,
                                             ds.stream));
    s.tmp_bytes = sort_need > scan_need ? sort_need : scan_need;
    ScratchLayout lay;
    const uint64_t o_canon = lay.add<fp256>(2 * (uint64_t)u);
    const uint64_t o_ss = lay.add<fp256>(u);
    const uint64_t o_keys = lay.add<uint64_t>(2 * (uint64_t)u);
    const uint64_t o_idx = lay.add<uint32_t>(7 * (uint64_t)u);
    const uint64_t o_words = lay.add<uint32_t>(LK_WORDS);
    const uint64_t o_tmp = lay.add<uint8_t>(s.tmp_bytes);
    RC_TRY(ds.d_call.reserve(lay.total));
    uint8_t* const a = ds.d_call.ptr;
    s.canon = (fp256*)(a + o_canon);
    s.ss = (fp256*)(a + o_ss);
    s.keys = (uint64_t*)(a + o_keys);
    s.idx = (uint32_t*)(a + o_idx);
    s.words = (uint32_t*)(a + o_words);
    s.tmp = a + o_tmp;
    return 0;
}

// LSD radix sort of one column's canonical values over the 64-bit limbs with
// end_bit[l] > 0; *perm_out = the sorted order (one of the two permutation
// arrays at the front of s.idx).
static int lk_sort_column(DeviceState& ds, const LkScratch& s,
                          const fp256* d_canon, uint32_t u,
                          const int end_bit[4], const uint32_t** perm_out) {
    uint64_t* keys_in = s.keys;
    uint64_t* keys_out = keys_in + u;
    uint32_t* cur = s.idx;
    uint32_t* nxt = cur + u;
    bool first = true;
    for (uint32_t l = 0; l < 4; l++) {
        if (!end_bit[l]) continue;
        if (first)
            hipLaunchKernelGGL(k_lk_limb_keys<true>, dim3(lk_blocks(u)),
                               dim3(LK_THREADS), 0, ds.stream,
                               (const uint64_t*)d_canon, l, cur, keys_in, u);
        else
            hipLaunchKernelGGL(k_lk_limb_keys<false>, dim3(lk_blocks(u)),
                               dim3(LK_THREADS), 0, ds.stream,
                               (const uint64_t*)d_canon, l, cur, keys_in, u);
        size_t tmp = s.tmp_bytes;
        CUB_TRY(hipcub::DeviceRadixSort::SortPairs(
            s.tmp, tmp, keys_in, keys_out, cur, nxt, (int64_t)u, 0,
            end_bit[l], ds.stream));
        uint32_t* t = cur;
        cur = nxt;
        nxt = t;
        first = false;
    }
    *perm_out = cur;
    return 0;
}

int fr_lookup_permute_device(spectre_gpu_ctx* ctx, int dev,
                             const fp256* d_input, const fp256* d_table,
                             fp256* d_input_perm, fp256* d_table_perm,
                             uint64_t u64) {
    if (u64 == 0) return 0;
    DeviceState& ds = ctx->devs[dev];
    HIP_TRY(hipSetDevice(ds.device_id));
    const uint32_t u = (uint32_t)u64;  // <= 2^28, checked by the caller
    LkScratch s;
    RC_TRY(lk_reserve(ds, u, s));
    hipStream_t st = ds.stream;
    fp256* canon_a = s.canon;  // later: canonical Ss
    fp256* canon_s = canon_a + u;
    fp256* ss_mont = s.ss;
    uint32_t* words = s.words;
    uint32_t* notfirst = s.idx + 2 * (size_t)u;
    uint32_t* free_ = notfirst + u;
    uint32_t* rank_rep = free_ + u;
    uint32_t* rank_left = rank_rep + u;
    uint32_t* rep = rank_left + u;
    const uint32_t nb = lk_blocks(u);

    // canonical copies and the OR of every limb
    HIP_TRY(hipMemsetAsync(words, 0, LK_WORDS * sizeof(uint32_t), st));
    const uint32_t cb = lk_blocks(2 * u);
    hipLaunchKernelGGL(k_lk_canon,
                       dim3(cb < LK_CANON_MAX_BLOCKS ? cb : LK_CANON_MAX_BLOCKS),
                       dim3(LK_THREADS), 0, st, d_input, d_table, canon_a, u,
                       words);
    uint32_t ors[LK_MISS];
    RC_TRY(call_finish(ds, ors, words, sizeof ors));
    // bits to sort per 64-bit limb; at least one pass, which also builds the
    // identity permutation when every value is zero
    int end_bit[4];
    bool any = false;
    for (int l = 0; l < 4; l++) {
        const uint64_t w = (uint64_t)ors[2 * l] | (uint64_t)ors[2 * l + 1] << 32;
        end_bit[l] = w ? 64 - __builtin_clzll(w) : 0;
        any |= w != 0;
    }
    if (!any) end_bit[0] = 1;

    const uint32_t* perm = nullptr;
    RC_TRY(lk_sort_column(ds, s, canon_a, u, end_bit, &perm));
    hipLaunchKernelGGL(k_lk_gather<false>, dim3(nb), dim3(LK_THREADS), 0, st,
                       d_input, (const fp256*)nullptr, perm, d_input_perm,
                       (fp256*)nullptr, u);
    RC_TRY(lk_sort_column(ds, s, canon_s, u, end_bit, &perm));
    // canonical A is dead: its half takes the canonical sorted table
    fp256* ss_canon = canon_a;
    hipLaunchKernelGGL(k_lk_gather<true>, dim3(nb), dim3(LK_THREADS), 0, st,
                       d_table, (const fp256*)canon_s, perm, ss_mont, ss_canon,
                       u);

    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)free_, 1, u, st));
    hipLaunchKernelGGL(k_lk_search, dim3(nb), dim3(LK_THREADS), 0, st,
                       (const fp256*)d_input_perm, (const fp256*)ss_canon, u,
                       notfirst, free_, words + LK_MISS);
    uint32_t missing = 0;
    RC_TRY(call_finish(ds, &missing, words + LK_MISS, sizeof missing));
    if (missing) {
        set_err("fr_lookup_permute: lookup miss: %u distinct input value%s "
                "absent from the table", missing, missing == 1 ? "" : "s");
        return SPECTRE_ERR_LOOKUP_MISS;
    }

    size_t tmp = s.tmp_bytes;
    CUB_TRY(hipcub::DeviceScan::ExclusiveSum(s.tmp, tmp, notfirst, rank_rep,
                                             (int)u, st));
    tmp = s.tmp_bytes;
    CUB_TRY(hipcub::DeviceScan::ExclusiveSum(s.tmp, tmp, free_, rank_left,
                                             (int)u, st));
    hipLaunchKernelGGL(k_lk_first_rows, dim3(nb), dim3(LK_THREADS), 0, st,
                       (const fp256*)d_input_perm, d_table_perm,
                       (const uint32_t*)notfirst, (const uint32_t*)rank_rep,
                       rep, u);
    hipLaunchKernelGGL(k_lk_fill, dim3(nb), dim3(LK_THREADS), 0, st,
                       (const fp256*)ss_mont, (const uint32_t*)free_,
                       (const uint32_t*)rank_left, (const uint32_t*)notfirst,
                       (const uint32_t*)rank_rep, (const uint32_t*)rep,
                       d_table_perm, u);
    return call_finish(ds);
}
