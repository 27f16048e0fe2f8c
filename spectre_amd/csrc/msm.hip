// msm.hip — BN254 G1 multi-scalar multiplication (Pippenger) for gfx950.
//
// Computes what halo2curves-axiom 0.5.2 `best_multiexp` computes (the value
// Sum_i k_i * P_i; windowing is free — see oracle/bn254.c header for the
// parity contract). The whole pipeline is batch-generic: `nbatch` scalar
// vectors over ONE shared base set run as a single sort/accumulate pass
// (create_proof commits ~17 advice columns against the same SRS back to
// back — SURVEY.md §8f-2); nbatch = 1 is the plain best_multiexp call.
//
// MI355X-native structure:
//   1. k_msm_digits     — one thread per point index: optional
//                         Montgomery->canonical conversion in registers,
//                         signed MSM_WBITS-bit window recoding, emit
//                         (bucket key, point index|sign) pairs for every
//                         (batch, window). Writes are (batch,window)-major,
//                         so each slice is written coalesced.
//   2. radix sort       — hipCUB DeviceRadixSort over batch*window*bucket
//                         keys; zero digits get a sentinel key sorting last.
//   3. k_bucket_offsets — binary-search segment bounds per bucket.
//   4. k_bucket_acc     — equal-work partitioning: each thread owns exactly
//                         E sorted entries, E chosen per call so small
//                         inputs still fill the chip (serial XYZZ+affine
//                         mixed adds, entry stream prefetched through LDS);
//                         interior runs write their bucket
//                         exclusively, boundary runs are merged by
//                         k_bucket_fix. Deterministic by construction, and
//                         the affine result is canonical, so ANY schedule
//                         yields bit-identical output bytes.
//   5. k_window_chunks  — per MSM_CHUNK consecutive buckets: plain sum T_c
//                         and locally weighted sum W_c from one suffix-sum
//                         loop. No per-chunk lift to the window offset.
//   6. k_window_tail    — three blocks per (batch, window) in one launch:
//                         sum of the W_c, and the row and column sums of the
//                         T_c (chunk index c = MSM_LO*hi + lo) weighted by
//                         their 6-bit index; serial adds, then a pairwise
//                         LDS tree. Buckets, chunk sums and the tree are
//                         XYZZ (g1.hpp); the thread that writes a partial
//                         converts it to Jacobian, the format of everything
//                         from here outward.
// Host side: msm_slot_drain folds the three partials of each window,
// P0 + CHUNK*(P1 + MSM_LO*P2) (9 doublings + 2 adds); ffi.cpp finishes each
// batch with the window Horner (~255 doublings + adds) and one field
// inversion to affine.
//
// All field math is 8x32-limb Montgomery (ff.hpp: the asm column multiply and
// squaring, add/sub/reduce as carry chains) — VALU integer work, issue-bound:
// in k_bucket_acc a third of the vector instructions are v_mad_u64_u32 and as
// many their carry adds (field add/sub section); MFMA does not
// apply to modular arithmetic.
#include "internal.hpp"
#include <hipcub/hipcub.hpp>

#define THREADS 256
// Point-arithmetic kernels hold a 32-VGPR XYZZ accumulator plus formula
// temporaries; at the default 4-waves/SIMD register budget (128 VGPR) hipcc
// spills to scratch. Allowing 2 waves/SIMD (256 VGPR) removes the spills —
// latency hiding comes from the serial-add structure, not occupancy
// (measured: 1 add-chain/thread already saturates the VALU issue pipe).
// With the carry-chain add/sub the kernels need 112-151 VGPRs (221 before)
// and run at 3-4 waves/SIMD under the same bound
// (profiles/xyzz_kernel_resources.txt).
#define PT_KERNEL __global__ __launch_bounds__(THREADS, 2)
// The accumulate/fix kernels have no barriers (k_bucket_acc's LDS staging
// is private to each wave, 8 KiB), so their block size only sets the
// residency granule. MEASURED (r2): 64/128/256-thread blocks
// are within run-to-run noise (acc 2.26-2.29 ms). The code object says
// k_bucket_acc uses 112 VGPRs (4 waves/SIMD; four blocks stage 128 KiB of a
// CU's 160 KiB of LDS). It had 165 (3 waves/SIMD) while ff_add / ff_sub were
// 64-bit limb code behind branches — the profiler's VGPR column shows half
// the allocation, which earlier notes misread as 4-5 waves/SIMD. One madd
// chain per SIMD already fills the issue pipe, so neither block size nor
// residency moves the stage. Kept tunable.
#ifndef MSM_ACC_THREADS
#define MSM_ACC_THREADS 256
#endif
#define ACC_KERNEL __global__ __launch_bounds__(MSM_ACC_THREADS, 2)

// ---- kernel 1: signed window decomposition --------------------------------
// w_lo/w_cnt: emit only windows [w_lo, w_lo+w_cnt) — window-sharded
// multi-GPU (each rank owns disjoint windows over ALL points, so bucket
// work AND the reduction tail divide by the rank count; the exchange is a
// pure allgather of disjoint window sums). The signed recoding carry runs
// over ALL windows regardless (it propagates from window 0 upward).
__global__ void k_msm_digits(const uint8_t* __restrict__ scalars, uint64_t n,
                             uint32_t nbatch, int canonical, uint32_t w_lo,
                             uint32_t w_cnt,
                             uint32_t* __restrict__ keys,
                             uint32_t* __restrict__ vals) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t nb_local = w_cnt * MSM_BPW;
    const uint32_t skip_key = nbatch * nb_local;
    for (uint32_t b = 0; b < nbatch; b++) {
        fp256 s;
        ff_from_bytes(s, scalars + 32 * (b * n + i));
        if (!canonical) ff_from_mont<Fr>(s, s);
        uint32_t carry = 0;
        for (int w = 0; w < MSM_NWIN; w++) {
            // c-bit window w of the canonical scalar (may cross limbs)
            const uint32_t bit0 = (uint32_t)w * MSM_WBITS;
            const uint32_t li = bit0 >> 5, sh = bit0 & 31;
            uint64_t pair = (uint64_t)s.l[li];
            if (li < 7) pair |= (uint64_t)s.l[li + 1] << 32;
            uint32_t d =
                ((uint32_t)(pair >> sh) & ((1u << MSM_WBITS) - 1)) + carry;
            const uint32_t half = 1u << (MSM_WBITS - 1);
            const uint32_t full = 1u << MSM_WBITS;
            uint32_t key, val = (uint32_t)i;
            if (d == 0) {
                carry = 0;
                key = skip_key;
            } else if (d <= half) {  // positive digit, magnitude d
                carry = 0;
                key = b * nb_local + ((uint32_t)w - w_lo) * MSM_BPW + (d - 1);
            } else if (d == full) {  // max digit + carry: digit 0, carry out
                carry = 1;
                key = skip_key;
            } else {  // negative digit, magnitude 2^c - d
                carry = 1;
                key = b * nb_local + ((uint32_t)w - w_lo) * MSM_BPW +
                      (full - d - 1);
                val |= 0x80000000u;
            }
            if ((uint32_t)w < w_lo || (uint32_t)w >= w_lo + w_cnt) continue;
            const uint64_t slot =
                ((uint64_t)b * w_cnt + ((uint32_t)w - w_lo)) * n + i;
            keys[slot] = key;
            vals[slot] = val;
        }
    }
}

// ---- kernel 3: per-bucket segment bounds via binary search ----------------
__global__ void k_bucket_offsets(const uint32_t* __restrict__ keys,
                                 uint64_t nent, uint32_t nb_total,
                                 uint32_t* __restrict__ off) {
    uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > nb_total) return;
    uint64_t lo = 0, hi = nent;
    while (lo < hi) {
        uint64_t mid = (lo + hi) >> 1;
        if (keys[mid] < b) lo = mid + 1;
        else hi = mid;
    }
    off[b] = (uint32_t)lo;
}

// ---- kernel 4: bucket accumulation, equal-work partitioning ---------------
// Bucket sizes are Poisson(mean ent/NB); one-thread-per-bucket makes the
// busiest lane in a wave ~1.5x the mean (SIMT runs at the max). Instead each
// thread owns exactly E consecutive SORTED entries (E is a per-call value,
// a multiple of 4 — see msm_acc_auto_entries): runs that start AND end
// strictly inside the range write their bucket directly (exclusive); the
// first and last (potentially thread-spanning) runs go to side arrays keyed
// by bucket, merged by k_bucket_fix.
//
// The entry stream is software-pipelined through LDS, so no global load sits
// between two madds and the prefetched data costs no registers (holding the
// next point in VGPRs across the madd dropped the 165-VGPR kernel to 2
// waves/SIMD; not retried at 111):
//   * keys/values arrive in 16-byte quads (thread ranges start at multiples
//     of 4 entries, so every quad is aligned), double-buffered: the quad
//     after the current one is in flight while the current one is consumed;
//   * the base point of entry i+1 is gathered BEFORE the madd of entry i,
//     from a value that is already in LDS.
// All of it uses the direct global->LDS load: each wave instruction writes
// 16 B per lane at (wave-uniform base + lane * 16), the source address is per
// lane. Per wave that is 8 KiB: 4 pieces of one affine point, 2x2 quads.
// Every prefetch stays inside the thread's own range: quads are only read
// while they hold at least one owned entry (the arrays are allocated in
// whole quads), points only for owned entries. All owned entries are real:
// off[nb_total] counts exactly the keys below the skip sentinel.
#define ACC_WAVES (MSM_ACC_THREADS / 64)
__device__ __forceinline__ void glds16(const void* src, uint4* wave_dst) {
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)src,
        (__attribute__((address_space(3))) void*)wave_dst, 16, 0, 0);
}
// direct loads landed / LDS reads returned (the compiler does not order
// either against the other kind of access to the same LDS bytes)
__device__ __forceinline__ void glds_landed() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
__device__ __forceinline__ void lds_reads_done() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

ACC_KERNEL void k_bucket_acc(const uint32_t* __restrict__ off,
                            const uint32_t* __restrict__ keys,
                            const uint32_t* __restrict__ vals,
                            const g1_affine* __restrict__ bases,
                            uint32_t nb_total, uint32_t E,
                            g1_xyzz* __restrict__ buckets,
                            uint32_t* __restrict__ firstK,
                            g1_xyzz* __restrict__ firstP,
                            uint32_t* __restrict__ lastK,
                            g1_xyzz* __restrict__ lastP) {
    // [wave][slot][lane]: slots 0-3 point x|y, 4-5 key quads, 6-7 value quads
    __shared__ uint4 stage[ACC_WAVES][8][64];
    const uint32_t ent = off[nb_total];  // real (non-skip) entries
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t lo = (uint64_t)t * E;
    if (lo >= ent) return;
    const uint32_t cnt = ent - lo < E ? (uint32_t)(ent - lo) : E;
    const uint4* kq = (const uint4*)(keys + lo);
    const uint4* vq = (const uint4*)(vals + lo);
    const uint32_t lane = threadIdx.x & 63;
    uint4(*st)[64] = stage[threadIdx.x >> 6];
    glds16(kq, st[4]);
    glds16(vq, st[6]);
    glds_landed();
    uint32_t k = st[4][lane].x;
    {
        // plain (cached) loads: bases are re-read by all 16 windows, so
        // L1/L2 residency pays (non-temporal loads measured 5% slower)
        const uint4* src = (const uint4*)(bases + (st[6][lane].x & 0x7fffffffu));
        for (int c = 0; c < 4; c++) glds16(src + c, st[c]);
    }
    // XYZZ (mADD-2008-s, 8M + 2S with Y3's two products under one
    // reduction), stored as it is: the flush below is a plain store. An
    // earlier XYZZ accumulator converted every finished run to Jacobian in
    // that branch (6M + 2S, issued by the whole wave whenever one lane ends a
    // run, about 87 % of iterations) and measured 2.31 -> 3.09 ms; without
    // the conversion this one is 9 % faster than the Jacobian madd
    // (XYZZ section).
    g1_xyzz acc;
    g1x_set_inf(acc);
    bool first = true;
    for (uint32_t i = 0; i < cnt; i++) {
        glds_landed();  // point i; quad issued at the previous multiple of 4
        const uint32_t q = 4 + ((i >> 2) & 1);
        const uint32_t kj = ((const uint32_t*)&st[q][lane])[i & 3];
        const uint32_t v = ((const uint32_t*)&st[q + 2][lane])[i & 3];
        g1_affine p;
        {
            const uint4 x0 = st[0][lane], x1 = st[1][lane];
            const uint4 y0 = st[2][lane], y1 = st[3][lane];
            p.x.l[0] = x0.x; p.x.l[1] = x0.y; p.x.l[2] = x0.z; p.x.l[3] = x0.w;
            p.x.l[4] = x1.x; p.x.l[5] = x1.y; p.x.l[6] = x1.z; p.x.l[7] = x1.w;
            p.y.l[0] = y0.x; p.y.l[1] = y0.y; p.y.l[2] = y0.z; p.y.l[3] = y0.w;
            p.y.l[4] = y1.x; p.y.l[5] = y1.y; p.y.l[6] = y1.z; p.y.l[7] = y1.w;
        }
        if (i + 1 < cnt) {
            const uint32_t qn = 6 + (((i + 1) >> 2) & 1);
            const uint32_t vn = ((const uint32_t*)&st[qn][lane])[(i + 1) & 3];
            lds_reads_done();  // before the slots read above are overwritten
            if ((i & 3) == 0 && i + 4 < cnt) {  // quad after the current one
                const uint32_t qf = 4 + (((i >> 2) + 1) & 1);
                glds16(kq + (i >> 2) + 1, st[qf]);
                glds16(vq + (i >> 2) + 1, st[qf + 2]);
            }
            const uint4* src = (const uint4*)(bases + (vn & 0x7fffffffu));
            for (int c = 0; c < 4; c++) glds16(src + c, st[c]);
        }
        if (kj != k) {  // flush completed run
            if (first) {
                firstK[t] = k;
                firstP[t] = acc;
                first = false;
            } else {
                buckets[k] = acc;  // interior run: exclusive writer
            }
            g1x_set_inf(acc);
            k = kj;
        }
        if (v & 0x80000000u) ff_neg<Fq>(p.y, p.y);
        g1x_madd_ip(acc, p);
    }
    if (first) {  // whole range is one run
        firstK[t] = k;
        firstP[t] = acc;
        lastK[t] = 0xffffffffu;
    } else {
        lastK[t] = k;
        lastP[t] = acc;
    }
}

// A point operand read whole, 16 bytes at a time, into registers before the
// add that consumes it. Handed a reference into memory, the inlined add loads
// each limb where a product first needs it and again at every later use, one
// dword and one wait at a time (the code object of k_window_chunks had 147
// global loads for its one 32-limb operand): in the fix, chunk and tail
// kernels, which run at one or two waves per SIMD, that latency is not hidden.
// The empty asm pins every limb in a VGPR, so the loads cannot sink.
__device__ __forceinline__ g1_xyzz pt_load(const g1_xyzz* src) {
    static_assert(sizeof(g1_xyzz) == 8 * sizeof(uint4), "four 32-byte elements");
    uint4 q[8];
#pragma unroll
    for (int i = 0; i < 8; i++) q[i] = ((const uint4*)src)[i];
#pragma unroll
    for (int i = 0; i < 8; i++)
        asm volatile("" : "+v"(q[i].x), "+v"(q[i].y), "+v"(q[i].z), "+v"(q[i].w));
    g1_xyzz v;
    memcpy(&v, q, sizeof v);
    return v;
}

// merge boundary partials: bucket b's segment [s,e) spans threads ts..te;
// interior-only buckets were already written by their exclusive thread.
ACC_KERNEL void k_bucket_fix(const uint32_t* __restrict__ off,
                            const uint32_t* __restrict__ firstK,
                            const g1_xyzz* __restrict__ firstP,
                            const uint32_t* __restrict__ lastK,
                            const g1_xyzz* __restrict__ lastP,
                            uint32_t nb_total, uint32_t E,
                            g1_xyzz* __restrict__ buckets) {
    uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb_total) return;
    uint32_t s = off[b], e = off[b + 1];
    if (s == e) {
        g1x_set_inf(buckets[b]);
        return;
    }
    uint32_t ts = s / E, te = (e - 1) / E;
    // interior (already written by its exclusive thread) iff the run starts
    // after the thread's range start AND ends before the thread's range end —
    // note a run ending at the END OF DATA (e == ent) ended the thread's
    // loop, so it lives in lastP, not in buckets[].
    const uint32_t ent = off[nb_total];
    if (ts == te && (s % E) && (e % E) && e != ent)
        return;
    g1_xyzz acc;
    g1x_set_inf(acc);
    for (uint32_t t = ts; t <= te; t++) {  // ascending = sorted entry order
        if (firstK[t] == b) g1x_add_ip(acc, pt_load(firstP + t));
        if (lastK[t] == b) g1x_add_ip(acc, pt_load(lastP + t));
    }
    buckets[b] = acc;
}

// ---- kernel 5: per-chunk sums ----------------------------------------------
// Window-local bucket j has multiplier (j+1). Chunk c of a window covers the
// window-local buckets [c*CHUNK, c*CHUNK+CHUNK); one thread per chunk forms,
// with one suffix-sum loop (two adds per bucket),
//   T_c = sum_j B[c*CHUNK+j]    and    W_c = sum_j (j+1) B[c*CHUNK+j].
// The chunk's offset in the window is NOT applied here: lifting T_c by
// c*CHUNK per chunk was half of this kernel's adds; kernel 6 applies the
// offsets to 2*64 marginal sums per window instead. Uniform in the flattened
// (batch*NWIN + w) window index, so batching needs no changes here.
PT_KERNEL void k_window_chunks(const g1_xyzz* __restrict__ buckets,
                               uint32_t total_chunks,
                               g1_xyzz* __restrict__ outW,
                               g1_xyzz* __restrict__ outT) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total_chunks) return;
    const g1_xyzz* B = buckets + (uint64_t)t * MSM_CHUNK;
    g1_xyzz accT, accW;
    g1x_set_inf(accT);
    g1x_set_inf(accW);
    for (int j = MSM_CHUNK - 1; j >= 0; j--) {
        g1x_add_ip(accT, pt_load(B + j));
        g1x_add_ip(accW, accT);
    }
    outW[t] = accW;
    outT[t] = accT;
}

// ---- kernel 6: per-window weighted sums -----------------------------------
// With c = MSM_LO*hi + lo the window sum is
//   sum_c W_c + CHUNK * ( sum_lo lo*R_lo + MSM_LO * sum_hi hi*C_hi ),
// R_lo = sum_hi T_(hi,lo) the column sums and C_hi = sum_lo T_(hi,lo) the row
// sums of the window's MSM_HI x MSM_LO grid of chunk totals. One block per
// (window, role) yields one of the three partials
//   role 0: P0 = sum_c W_c     role 1: P1 = sum_lo lo*R_lo
//   role 2: P2 = sum_hi hi*C_hi
// and the host folds them (msm_fold_window). All roles run the same code:
// every thread sums its share serially (thread t = q*M + idx takes a q-th
// of marginal idx, M = MSM_LO or MSM_HI marginals; role 0 grid-strides), a
// pairwise LDS tree halves the live threads per level, and at the level
// where M threads are left — each holding marginal idx = t — roles 1 and 2
// multiply by idx with a log2(M)-bit double-and-add. Serial depth at
// CHUNK = 8 with 512 threads (8 per marginal): 8 adds + 3 levels + a 6-bit
// multiply (about 6) + 6 levels, about 23 add-equivalents, in ONE launch of
// 3 blocks per window (a 3-level cascade of tiny grids was ~0.8 ms of
// launch+latency overhead). Empty marginals skip their multiply, and every
// add returns early on the identity.
// MEASURED on MI355X: 512 against 256 threads (16 adds + 2 levels first)
// takes the stage from 0.74 to 0.61 ms at every n and one synchronous call
// at n = 2^12 from 1.42 to 1.31 ms; the pipelined throughput at n = 2^20 is
// the same within its noise. 512 threads is two waves on each SIMD of a CU,
// within the 256-VGPR budget (the kernel has 140 VGPRs, 220 before the
// carry-chain add/sub). The tree's XYZZ elements take 32 KiB of LDS.
#ifndef WSUM_THREADS
#define WSUM_THREADS 512
#endif
static_assert(MSM_CPW % WSUM_THREADS == 0, "role 0 shares");
static_assert(WSUM_THREADS % MSM_LO == 0 && MSM_HI % (WSUM_THREADS / MSM_LO) == 0,
              "column shares");
static_assert(MSM_HI <= WSUM_THREADS && WSUM_THREADS % MSM_HI == 0 &&
              MSM_LO % (WSUM_THREADS / MSM_HI) == 0, "row shares");
__global__ __launch_bounds__(WSUM_THREADS, 2) void k_window_tail(
    const g1_xyzz* __restrict__ inW, const g1_xyzz* __restrict__ inT,
    g1_jac* __restrict__ out) {
    __shared__ __align__(16) g1_xyzz lds[WSUM_THREADS / 2];  // pt_load: 16 B
    const uint32_t w = blockIdx.x / 3, role = blockIdx.x % 3;
    const uint32_t t = threadIdx.x;
    // marginals of this role, and this thread's share: cnt elements from
    // src, stride apart
    const uint32_t M = role == 0 ? 0 : role == 1 ? MSM_LO : MSM_HI;
    const g1_xyzz* src;
    uint32_t stride, cnt;
    if (role == 0) {
        src = inW + (uint64_t)w * MSM_CPW + t;
        stride = WSUM_THREADS;
        cnt = MSM_CPW / WSUM_THREADS;
    } else if (role == 1) {  // column lo = t % LO, rows [q*cnt, q*cnt+cnt)
        cnt = MSM_HI / (WSUM_THREADS / MSM_LO);
        src = inT + (uint64_t)w * MSM_CPW + (t / MSM_LO) * cnt * MSM_LO +
              t % MSM_LO;
        stride = MSM_LO;
    } else {  // row hi = t % HI, columns [q*cnt, q*cnt+cnt)
        cnt = MSM_LO / (WSUM_THREADS / MSM_HI);
        src = inT + (uint64_t)w * MSM_CPW + (t % MSM_HI) * MSM_LO +
              (t / MSM_HI) * cnt;
        stride = 1;
    }
    g1_xyzz acc;
    g1x_set_inf(acc);
    for (uint32_t j = 0; j < cnt; j++)
        g1x_add_ip(acc, pt_load(src + (uint64_t)j * stride));
    for (uint32_t k = WSUM_THREADS / 2; k >= 1; k >>= 1) {
        if (2 * k == M && t < M) {  // acc = marginal t: acc *= t
            if (t == 0) g1x_set_inf(acc);
            if (!g1x_is_inf(acc)) {
                g1_xyzz r;
                g1x_set_inf(r);
                for (uint32_t bit = M >> 1; bit; bit >>= 1) {
                    g1x_dbl_ip(r);
                    if (t & bit) g1x_add_ip(r, acc);
                }
                acc = r;
            }
        }
        if (t >= k && t < 2 * k) lds[t - k] = acc;
        __syncthreads();
        if (t < k) g1x_add_ip(acc, pt_load(lds + t));
        __syncthreads();
    }
    // the one conversion: the partials leave in the 96-byte Jacobian format
    if (t == 0) g1x_to_jac(out[blockIdx.x], acc);
}

// ---- host orchestration ---------------------------------------------------
// Entries per accumulate thread when the caller has not fixed one.
// MEASURED on MI355X (n = 2^20, accumulate + fix stage): one madd chain per
// SIMD already fills the issue pipe, so the stage costs the
// same 2.23-2.25 ms for E = 32, 44, 64 whether or not the grid is a whole
// number of resident rounds, and MORE for one exact round (E = 88: 2.38 ms;
// half a round, E = 176: 3.16 ms): the dispatcher balances many short
// blocks better than equal shares balance themselves. So large inputs keep
// E = MSM_ACC_E_MAX. Small inputs are where E matters: at n = 2^16 the
// stage takes 0.91 ms at E = 64 (64 blocks on 256 CUs), 0.52 at 32, 0.32 at
// 16, 0.29 at 8 and 0.37 at 4, where the two boundary partials per thread
// that k_bucket_fix merges start to cost more than the parallelism gives.
// Measured again with the carry-chain add/sub (every figure about a fifth
// lower, the same ordering: 1.85 / 1.87 / 1.96 ms at E = 64 / 32 / 88;
// 0.70 / 0.40 / 0.24 / 0.24 / 0.27 at n = 2^16): the rule stands
// (profiles/field_chain_sweeps.txt).
// The rule: aim for MSM_ACC_TARGET_BLOCKS resident blocks on every CU
// (fewer if fewer fit), E rounded up to the quad the kernel loads, within
// [MSM_ACC_E_MIN, MSM_ACC_E_MAX].
uint32_t msm_acc_auto_entries(uint64_t entries, uint32_t cus,
                              uint32_t resident_blocks) {
    uint32_t per_cu = resident_blocks ? resident_blocks : 1;
    if (per_cu > MSM_ACC_TARGET_BLOCKS) per_cu = MSM_ACC_TARGET_BLOCKS;
    const uint64_t threads =
        (uint64_t)(cus ? cus : 1) * per_cu * MSM_ACC_THREADS;
    if (entries >= threads * MSM_ACC_E_MAX) return MSM_ACC_E_MAX;
    uint64_t e = (entries + threads - 1) / threads;
    e = (e + 3) & ~3ull;
    if (e < MSM_ACC_E_MIN) e = MSM_ACC_E_MIN;
    if (e > MSM_ACC_E_MAX) e = MSM_ACC_E_MAX;
    return (uint32_t)e;
}

// CUs and resident k_bucket_acc blocks per CU, once per device.
static int ensure_acc_geometry(DeviceState& dstate) {
    if (dstate.acc_resident_blocks) return 0;
    int cus = 0, nb = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                                  dstate.device_id));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &nb, k_bucket_acc, MSM_ACC_THREADS, 0));
    dstate.num_cus = cus > 0 ? cus : 1;
    dstate.acc_resident_blocks = nb > 0 ? nb : 1;
    return 0;
}

static int ensure_msm_scratch(MsmSlot& ds, uint64_t ent, uint32_t nwin,
                              uint32_t acc_e) {
    const uint64_t nbt = (uint64_t)nwin * MSM_BPW;
    // Each group is reserved with one size, so its members grow together; a
    // group left half-grown by a failed allocation is finished by the next
    // call (every buffer carries its own capacity).
    // whole quads: k_bucket_acc reads keys/values 16 bytes at a time
    const uint64_t ent4 = (ent + 3) & ~3ull;
    for (auto* b : {&ds.d_keys_in, &ds.d_keys_out, &ds.d_vals_in,
                    &ds.d_vals_out})
        RC_TRY(b->reserve(ent4));
    // boundary-run side arrays: one slot per accumulate thread of THIS call
    const uint64_t nt = (ent + acc_e - 1) / acc_e;
    RC_TRY(ds.d_firstK.reserve(nt));
    RC_TRY(ds.d_lastK.reserve(nt));
    RC_TRY(ds.d_firstP.reserve(nt));
    RC_TRY(ds.d_lastP.reserve(nt));
    RC_TRY(ds.d_offsets.reserve(nbt + 1));
    RC_TRY(ds.d_buckets.reserve(nbt));
    RC_TRY(ds.d_red.reserve(2 * nbt / MSM_CHUNK));
    RC_TRY(ds.d_part.reserve(3 * (uint64_t)nwin));
    size_t sort_need = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(
        nullptr, sort_need, ds.d_keys_in.ptr, ds.d_keys_out.ptr,
        ds.d_vals_in.ptr, ds.d_vals_out.ptr, (int64_t)ent, 0, 32, ds.stream);
    return ds.d_sort_tmp.reserve(sort_need);
}

static int end_bit_for(uint64_t max_key) {
    int b = 0;
    while ((1ull << b) <= max_key) b++;
    return b;
}

// Per-stage HIP events on the slot's stream (the live in-bench measurement
// the roofline report is built from). Events exist only when timing was
// asked for and are destroyed on every return path.
struct StageTimer {
    hipEvent_t ev[7] = {};
    hipStream_t st = nullptr;
    hipError_t err = hipSuccess;  // first failed record, reported by read()
    uint32_t ent_real = 0;        // non-zero-digit entries (off[nbt])
    bool on = false;
    ~StageTimer() {
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int start(hipStream_t s) {
        on = true;
        st = s;
        for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
        return 0;
    }
    void stamp(int i) {
        if (on && err == hipSuccess) err = hipEventRecord(ev[i], st);
    }
    int read(double* stage_ms) {  // after the stream has been synchronized
        HIP_TRY(err);
        float ms;
        for (int i = 0; i < 6; i++) {
            HIP_TRY(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            stage_ms[i] = ms;
        }
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[6]));
        stage_ms[6] = ms;
        stage_ms[7] = (double)ent_real;
        return 0;
    }
};

// Validate the call and hand out its slot (stream created on first use).
static int msm_acquire_slot(DeviceState& dstate, const MsmCall& c, int slot,
                            MsmSlot** out) {
    HIP_TRY(hipSetDevice(dstate.device_id));
    if (slot < 0 || slot >= MSM_SLOTS) {
        set_err("msm: slot %d out of range", slot);
        return -3;
    }
    MsmSlot& ds = dstate.slots[slot];
    if (ds.pending_dst) {
        // a second call on a busy slot, synchronous or not, would overwrite
        // the pinned window sums of the pending one silently — fail loudly
        // instead (callers must slot_wait first)
        set_err("msm: slot %d already has a call in flight", slot);
        return -3;
    }
    if (!ds.stream) {
        if (slot == 0) ds.stream = dstate.stream;
        else HIP_TRY(hipStreamCreate(&ds.stream));
    }
    if (c.nbatch == 0 || c.nbatch > SPECTRE_MSM_MAX_BATCH) {
        set_err("msm: nbatch %u out of range [1,%d]", c.nbatch,
                SPECTRE_MSM_MAX_BATCH);
        return -3;
    }
    if (c.w_lo >= MSM_NWIN || c.w_cnt == 0 || c.w_lo + c.w_cnt > MSM_NWIN) {
        set_err("msm: window range [%u, %u+%u) out of [0,%d)", c.w_lo, c.w_lo,
                c.w_cnt, MSM_NWIN);
        return -3;
    }
    // Sort entries and segment offsets are indexed with uint32: at exactly
    // nbatch*NWIN*n == 2^32 the final offset off[nb_total] wraps to 0 and the
    // result is silently wrong. Reject; callers split such jobs (e.g. batch
    // 32 x 2^23 -> 2 x 16).
    if ((uint64_t)c.nbatch * c.w_cnt * c.n >= (1ull << 32)) {
        set_err("msm: nbatch*%u*n = %llu exceeds 2^32 sort-entry limit "
                "(split the batch or shard the MSM)", c.w_cnt,
                (unsigned long long)((uint64_t)c.nbatch * c.w_cnt * c.n));
        return -3;
    }
    *out = &ds;
    return 0;
}

// Size the slot's scratch, launch the six stages and the D2H of the window
// partials into the slot's pinned buffer, and mark the slot busy:
// msm_slot_drain folds them into the window sums in winsums_host.
static int msm_enqueue(spectre_gpu_ctx* ctx, DeviceState& dstate, MsmSlot& ds,
                       const MsmCall& c, g1_jac* winsums_host,
                       StageTimer& timer) {
    const uint32_t nw = c.nbatch * c.w_cnt;
    const uint64_t ent = (uint64_t)nw * c.n;
    RC_TRY(ensure_acc_geometry(dstate));
    const uint32_t acc_e =
        ctx->msm_acc_entries
            ? ctx->msm_acc_entries
            : msm_acc_auto_entries(ent, (uint32_t)dstate.num_cus,
                                   (uint32_t)dstate.acc_resident_blocks);
    RC_TRY(ensure_msm_scratch(ds, ent, nw, acc_e));
    RC_TRY(ds.h_wins.reserve(3 * (size_t)nw));
    const uint32_t nbt = nw * MSM_BPW;
    const int canonical = (c.flags & SPECTRE_SCALARS_CANONICAL) ? 1 : 0;
    hipStream_t st = ds.stream;

    timer.stamp(0);
    uint32_t blocks = (uint32_t)((c.n + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(k_msm_digits, dim3(blocks), dim3(THREADS), 0, st,
                       c.d_scalars, c.n, c.nbatch, canonical, c.w_lo, c.w_cnt,
                       ds.d_keys_in.ptr, ds.d_vals_in.ptr);
    timer.stamp(1);
    size_t tmp = ds.d_sort_tmp.cap;
    (void)hipcub::DeviceRadixSort::SortPairs(
        ds.d_sort_tmp.ptr, tmp, ds.d_keys_in.ptr, ds.d_keys_out.ptr,
        ds.d_vals_in.ptr, ds.d_vals_out.ptr, (int64_t)ent, 0,
        end_bit_for(nbt), st);
    timer.stamp(2);
    hipLaunchKernelGGL(k_bucket_offsets,
                       dim3((nbt + 1 + THREADS - 1) / THREADS), dim3(THREADS),
                       0, st, ds.d_keys_out.ptr, ent, nbt, ds.d_offsets.ptr);
    timer.stamp(3);
    const uint32_t nt_acc = (uint32_t)((ent + acc_e - 1) / acc_e);
    hipLaunchKernelGGL(k_bucket_acc,
                       dim3((nt_acc + MSM_ACC_THREADS - 1) / MSM_ACC_THREADS),
                       dim3(MSM_ACC_THREADS), 0, st, ds.d_offsets.ptr,
                       ds.d_keys_out.ptr, ds.d_vals_out.ptr, c.d_bases, nbt,
                       acc_e, ds.d_buckets.ptr, ds.d_firstK.ptr,
                       ds.d_firstP.ptr, ds.d_lastK.ptr, ds.d_lastP.ptr);
    hipLaunchKernelGGL(k_bucket_fix,
                       dim3((nbt + MSM_ACC_THREADS - 1) / MSM_ACC_THREADS),
                       dim3(MSM_ACC_THREADS), 0, st, ds.d_offsets.ptr,
                       ds.d_firstK.ptr, ds.d_firstP.ptr, ds.d_lastK.ptr,
                       ds.d_lastP.ptr, nbt, acc_e, ds.d_buckets.ptr);
    timer.stamp(4);
    const uint32_t nchunks = nbt / MSM_CHUNK;
    g1_xyzz* redW = ds.d_red.ptr;
    g1_xyzz* redT = redW + nchunks;
    g1_jac* redP = ds.d_part.ptr;  // 3 partials per window
    hipLaunchKernelGGL(k_window_chunks,
                       dim3((nchunks + THREADS - 1) / THREADS), dim3(THREADS),
                       0, st, ds.d_buckets.ptr, nchunks, redW, redT);
    timer.stamp(5);
    hipLaunchKernelGGL(k_window_tail, dim3(3 * nw), dim3(WSUM_THREADS), 0, st,
                       redW, redT, redP);
    timer.stamp(6);
    HIP_TRY(hipMemcpyAsync(ds.h_wins.ptr, redP,
                           3 * (size_t)nw * sizeof(g1_jac),
                           hipMemcpyDeviceToHost, st));
    if (timer.on)
        HIP_TRY(hipMemcpyAsync(&timer.ent_real, ds.d_offsets.ptr + nbt, 4,
                               hipMemcpyDeviceToHost, st));
    HIP_TRY(hipGetLastError());
    ds.pending_dst = winsums_host;
    ds.pending_n = nw;
    return 0;
}

// window = p0 + CHUNK * (p1 + LO * p2): log2(LO) + log2(CHUNK) doublings and
// two adds (host build of g1.hpp).
void msm_fold_window(const g1_jac& p0, const g1_jac& p1, const g1_jac& p2,
                     g1_jac& out) {
    g1_jac acc = p2;
    for (uint32_t m = MSM_LO; m > 1; m >>= 1) g1j_dbl_ip(acc);
    g1j_add_ip(acc, p1);
    for (uint32_t m = MSM_CHUNK; m > 1; m >>= 1) g1j_dbl_ip(acc);
    g1j_add_ip(acc, p0);
    out = acc;
}

// Synchronize a slot's stream, fold the pending window partials (pinned) and
// deliver the window sums (-> caller memory). Idempotent when nothing is
// pending. The hand-off is cleared on the error returns too: a failed drain
// leaves neither a wedged slot nor a destination that may since have been
// freed.
int msm_slot_drain(spectre_gpu_ctx* ctx, int dev, int slot) {
    DeviceState& dstate = ctx->devs[dev];
    if (slot < 0 || slot >= MSM_SLOTS) {
        set_err("slot_drain: slot %d out of range", slot);
        return -1;
    }
    MsmSlot& sl = dstate.slots[slot];
    g1_jac* const dst = sl.pending_dst;
    const uint32_t nw = sl.pending_n;
    sl.pending_dst = nullptr;
    sl.pending_n = 0;
    HIP_TRY(hipSetDevice(dstate.device_id));
    if (sl.stream) HIP_TRY(hipStreamSynchronize(sl.stream));
    HIP_TRY(hipGetLastError());
    if (dst) {
        const g1_jac* p = sl.h_wins.ptr;
        for (uint32_t w = 0; w < nw; w++, p += 3) {
            g1_jac sum;
            msm_fold_window(p[0], p[1], p[2], sum);
            // caller memory of any alignment
            memcpy((uint8_t*)dst + w * sizeof sum, &sum, sizeof sum);
        }
    }
    return 0;
}

int msm_device(spectre_gpu_ctx* ctx, int dev, const MsmCall& call,
               g1_jac* winsums_host, double* stage_ms, bool sync, int slot) {
    DeviceState& dstate = ctx->devs[dev];
    MsmSlot* sl = nullptr;
    RC_TRY(msm_acquire_slot(dstate, call, slot, &sl));
    if (call.n == 0) {
        for (uint32_t w = 0; w < call.nbatch * call.w_cnt; w++)
            g1j_set_inf(winsums_host[w]);
        return 0;
    }
    StageTimer timer;
    if (stage_ms) RC_TRY(timer.start(sl->stream));
    RC_TRY(msm_enqueue(ctx, dstate, *sl, call, winsums_host, timer));
    if (!sync && !stage_ms) return 0;  // completed by msm_slot_drain
    RC_TRY(msm_slot_drain(ctx, dev, slot));
    return stage_ms ? timer.read(stage_ms) : 0;
}
