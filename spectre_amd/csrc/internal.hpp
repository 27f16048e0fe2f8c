// internal.hpp — shared internals of libspectre_gpu.so (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include "spectre_gpu.h"
#include "ff.hpp"
#include "g1.hpp"
#include "powtab.hpp"
#include <array>
#include <map>
#include <mutex>
#include <string>
#include <vector>

// MSM window configuration: MSM_NWIN signed MSM_WBITS-bit windows covering
// >= 255 bits. Signed-digit recoding halves the bucket count: digit
// magnitudes in [1, 2^(WBITS-1)], bucket index = magnitude-1, negative
// digits negate the point (one Fq negation). Canonical BN254 Fr scalars are
// < 2^254 and NWIN*WBITS >= 255, so the top window never recodes negative
// and never carries out. Measured on MI355X: c=15 trades +8% bucket work
// for a 2x smaller tail and nets out slightly WORSE than c=16 (5.14 vs
// 5.02 ms at n=2^20) - c=16 kept.
#define MSM_WBITS 16
#define MSM_NWIN 16                        // ceil(255 / WBITS)
#define MSM_BPW (1u << (MSM_WBITS - 1))    // buckets per window
#ifndef MSM_CHUNK
#define MSM_CHUNK SPECTRE_MSM_TAIL_CHUNK   // buckets per reduction thread
#endif
// The reduction tail splits a window's chunk index c = MSM_LO * hi + lo and
// weights the row and column sums of the chunk totals instead of lifting
// every chunk on its own (msm.hip, kernels 5 and 6).
#define MSM_CPW (MSM_BPW / MSM_CHUNK)      // chunks per window
#define MSM_LO SPECTRE_MSM_TAIL_LO         // columns of the chunk grid
#define MSM_HI (MSM_CPW / MSM_LO)          // rows of the chunk grid
static_assert(MSM_CPW % MSM_LO == 0, "chunks per window: a multiple of MSM_LO");
static_assert((MSM_CHUNK & (MSM_CHUNK - 1)) == 0 && (MSM_LO & (MSM_LO - 1)) == 0,
              "the host fold multiplies by doubling");
// Sorted entries per accumulate thread are a per-call value (a multiple of
// 4): ctx->msm_acc_entries when set, else msm_acc_auto_entries() within
// these bounds.
#define MSM_ACC_E_MIN 8
#define MSM_ACC_E_MAX 64
#define MSM_ACC_TARGET_BLOCKS 2            // accumulate blocks aimed at per CU

void set_err(const char* fmt, ...);

#define HIP_TRY(x)                                                        \
    do {                                                                  \
        hipError_t _e = (x);                                              \
        if (_e != hipSuccess) {                                           \
            set_err("%s:%d %s: %s", __FILE__, __LINE__, #x,               \
                    hipGetErrorString(_e));                               \
            return -2;                                                    \
        }                                                                 \
    } while (0)

// propagate a nonzero return code
#define RC_TRY(x)                                                         \
    do {                                                                  \
        int _rc = (x);                                                    \
        if (_rc) return _rc;                                              \
    } while (0)

// Growable scratch: a pointer and its capacity in elements, in device memory
// or (kPinned) pinned host memory. Growth frees first and never preserves
// contents; the pointer is null and the capacity 0 until an allocation has
// succeeded, so a failed reserve() leaves nothing dangling. Plain data on
// purpose (DeviceState is copied into ctx->devs); owners call release()
// with the right device current.
template <typename T, bool kPinned = false>
struct DevBuf {
    T* ptr = nullptr;
    size_t cap = 0;  // elements
    int reserve(size_t n) {
        if (cap >= n) return 0;
        release();
        void* p = nullptr;
        if (kPinned) HIP_TRY(hipHostMalloc(&p, n * sizeof(T)));
        else HIP_TRY(hipMalloc(&p, n * sizeof(T)));
        ptr = (T*)p;
        cap = n;
        return 0;
    }
    void release() {
        if (ptr) (void)(kPinned ? hipHostFree(ptr) : hipFree(ptr));
        ptr = nullptr;
        cap = 0;
    }
};
template <typename T>
using PinnedBuf = DevBuf<T, true>;
template <typename... B>
void release_all(B&... b) {
    (b.release(), ...);
}

// Cached across calls, so a plan owns its tables (twB too: not in d_call).
struct NttPlan {
    uint32_t npass = 0;      // axes of the split, one global pass each
    uint32_t k[3] = {};      // log2 axis sizes; the last is the contiguous one
    DevBuf<fp256> tw[3];     // butterfly twiddles per axis, 2^(k-1) entries
    DevBuf<fp256> twB;       // the omega-power table (powtab.hpp), e < n
    PowTable omega = {};     // its two halves
    void release() { release_all(tw[0], tw[1], tw[2], twB); }
};

// Per-slot MSM pipeline state: MSM_SLOTS slots per device let call i+1's
// digits/sort/accumulate fill the machine while call i's latency-bound
// reduction tail (~1.3 ms at <=1 wave/SIMD) drains on another stream —
// back-to-back commits (create_proof issues ~45 per proof) overlap instead
// of serializing on the tail. Sizes below are per call: ent = nbatch *
// w_cnt * n sort entries, nbt = nbatch * w_cnt * MSM_BPW buckets.
#define MSM_SLOTS 3  // >=2 enables the async pipeline; 3rd for depth-3 A/B
struct MsmSlot {
    hipStream_t stream = nullptr;  // slot 0 aliases DeviceState::stream
    // sort keys/values, ent rounded up to whole quads; grow together
    DevBuf<uint32_t> d_keys_in, d_keys_out, d_vals_in, d_vals_out;
    DevBuf<uint8_t> d_sort_tmp;  // radix-sort temp storage (bytes)
    // boundary-run side arrays, one entry per accumulate thread
    // (ceil(ent / entries-per-thread)); grow together
    DevBuf<uint32_t> d_firstK, d_lastK;
    DevBuf<g1_xyzz> d_firstP, d_lastP;
    // grow together:
    DevBuf<uint32_t> d_offsets;  // nbt + 1 segment bounds
    DevBuf<g1_xyzz> d_buckets;   // nbt
    DevBuf<g1_xyzz> d_red;       // nbt/MSM_CHUNK weighted chunk sums W, then
                                 // as many plain chunk sums T
    DevBuf<g1_jac> d_part;       // three partials for each of nbatch * w_cnt
                                 // windows, Jacobian like everything outward
    // The window partials (3 per window) come back through a PINNED per-slot
    // buffer: an async D2H into caller (pageable) memory silently blocks the
    // calling thread on ROCm, which serialized the whole slot pipeline in
    // r2's first measurement. msm_slot_drain folds pinned -> caller.
    PinnedBuf<g1_jac> h_wins;
    // Result hand-off, set by the enqueue and cleared by msm_slot_drain
    // (msm.hip) and nowhere else; non-null = the slot is busy.
    g1_jac* pending_dst = nullptr;  // caller buffer for the in-flight call
    uint32_t pending_n = 0;         // elements pending (nbatch * w_cnt)
    void release(hipStream_t shared) {
        release_all(d_keys_in, d_keys_out, d_vals_in, d_vals_out, d_sort_tmp,
                    d_firstK, d_lastK, d_firstP, d_lastP, d_offsets,
                    d_buckets, d_red, d_part, h_wins);
        if (stream && stream != shared) (void)hipStreamDestroy(stream);
        stream = nullptr;
    }
};

struct DeviceState {
    int device_id = 0;
    hipStream_t stream = nullptr;
    MsmSlot slots[MSM_SLOTS];
    int next_slot = 0;  // round-robin for the async API
    int num_cus = 0;              // filled with acc_resident_blocks
    int acc_resident_blocks = 0;  // k_bucket_acc blocks resident per CU
    // ---- caller data held across a nested device call (a host-pointer
    // entry point uploads, then calls the device one, which carves up
    // d_call), so not part of d_call ----
    DevBuf<uint8_t> d_scalars;   // host-pointer MSM scratch (bytes)
    DevBuf<g1_affine> d_bases;   // uncached host-pointer bases (points)
    // key = (bases_id, n, shard layout): layout is num_gpus for the sharded
    // path (this device's contiguous chunk of an n-point set split num_gpus
    // ways) and 1 for the full set (batch path == num_gpus=1 shard).
    std::map<std::array<uint64_t, 3>, DevBuf<g1_affine>> bases_cache;
    DevBuf<fp256> d_ntt_io;   // cached device buffer for host-pointer NTTs
                              // (the Rust seam calls this path ~40-60x per
                              // proof; no per-call hipMalloc)
    // ---- pinned staging for host-pointer uploads/downloads ----
    PinnedBuf<uint8_t> h_stage[2];
    hipEvent_t stage_ev[2] = {nullptr, nullptr};
    // ---- the call arena: all device scratch of the synchronous Fr calls
    // (ntt, gate, poly, lookup, perm .hip), laid out per call with a
    // ScratchLayout (scratch.hpp). Every user holds ctx->mu; reserves its
    // whole call ONCE, before its first launch (growth frees the buffer: a
    // second reserve would pull it out from under pointers kernels already
    // hold); synchronizes the stream before it returns (call_finish); and
    // keeps no pointer into it across calls. So no two users are live at
    // once and the device holds the largest call's need, not the sum. The
    // MSM slots are asynchronous and outlive the call: not in it. ----
    DevBuf<uint8_t> d_call;
    // pinned landing spot of a call's readback (call_finish), reserved on
    // first use
    PinnedBuf<uint8_t> h_call;
    std::map<std::array<uint8_t, 40>, NttPlan> plans;  // omega||log_n
    // frees everything this device owns; the caller has made it current
    void release() {
        for (auto& sl : slots) sl.release(stream);
        release_all(d_scalars, d_bases, d_ntt_io, h_stage[0], h_stage[1],
                    d_call, h_call);
        for (auto& kv : bases_cache) kv.second.release();
        bases_cache.clear();
        for (auto& kv : plans) kv.second.release();
        plans.clear();
        for (auto& e : stage_ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
    }
};

// The one epilogue of a synchronous device call: if dst is given, enqueue
// the readback of bytes <= CALL_PINNED_BYTES from d_src into h_call; then
// synchronize the stream, surface a launch error, and copy the bytes out.
// The largest readback is fr_poly_eval_batch's: 32 polynomials at 8 points.
#define CALL_PINNED_BYTES \
    (SPECTRE_OPEN_MAX_POLYS * SPECTRE_POLY_EVAL_MAX_POINTS * 32u)
inline int call_finish(DeviceState& ds, void* dst = nullptr,
                       const void* d_src = nullptr, size_t bytes = 0) {
    if (dst) {
        RC_TRY(ds.h_call.reserve(CALL_PINNED_BYTES));
        HIP_TRY(hipMemcpyAsync(ds.h_call.ptr, d_src, bytes,
                               hipMemcpyDeviceToHost, ds.stream));
    }
    HIP_TRY(hipStreamSynchronize(ds.stream));
    HIP_TRY(hipGetLastError());
    if (dst) memcpy(dst, ds.h_call.ptr, bytes);
    return 0;
}

struct spectre_gpu_ctx {
    std::vector<DeviceState> devs;
    std::recursive_mutex mu;
    uint32_t msm_acc_entries = 0;  // entries per accumulate thread, 0 = auto
    uint32_t fr_scan_tile = 0;     // elements per poly.hip tile, 0 = default
    bool ntt_force3 = false;       // three-axis NTT split at every log_n >= 3
};

// One MSM pipeline run: nbatch scalar vectors (batch-major, nbatch*n*32 B)
// over one shared base set, restricted to windows [w_lo, w_lo+w_cnt).
// Full-range callers pass 0, MSM_NWIN. In a window shard the bucket work AND
// the reduction tail divide by the shard count; the carry recoding still
// runs over all windows.
struct MsmCall {
    const g1_affine* d_bases;
    const uint8_t* d_scalars;
    uint32_t nbatch;
    uint64_t n;
    uint32_t flags;
    uint32_t w_lo, w_cnt;
};

// msm.hip — the one MSM device entry point: runs the Pippenger pipeline for
// `call` on pipeline slot `slot` (scratch + stream; streams of slots > 0 are
// created lazily) of device `dev`; winsums_host receives nbatch * w_cnt
// Jacobian window sums. A slot with a result pending rejects every call.
// sync=false: enqueue the pipeline and the D2H of the sums and return; the
// sums are delivered by msm_slot_drain (multi-device / pipelined overlap).
// stage_ms != nullptr (always synchronizes): per-stage HIP-event timings
// [0]=digits [1]=sort [2]=offsets [3]=bucket_acc [4]=chunks [5]=reduce
// [6]=total-gpu [7]=real (non-zero-digit) entry count.
int msm_device(spectre_gpu_ctx* ctx, int dev, const MsmCall& call,
               g1_jac* winsums_host, double* stage_ms, bool sync, int slot);

// msm.hip — the auto rule for entries per accumulate thread (pure; host).
uint32_t msm_acc_auto_entries(uint64_t entries, uint32_t cus,
                              uint32_t resident_blocks);

// msm.hip — sync a slot's stream, fold the pending window partials and
// deliver the window sums.
int msm_slot_drain(spectre_gpu_ctx* ctx, int dev, int slot);

// msm.hip — one window sum from the three partials the device tail yields:
// out = p0 + MSM_CHUNK * (p1 + MSM_LO * p2) (pure; host). out may alias an
// input.
void msm_fold_window(const g1_jac& p0, const g1_jac& p1, const g1_jac& p2,
                     g1_jac& out);

// gate.hip — gate-expression evaluator over device column buffers
// (synchronizes). cols = host array of ncols device pointers.
int fr_gate_eval_device(spectre_gpu_ctx* ctx, int dev,
                        const fp256* const* cols, uint32_t ncols,
                        const fp256* consts, uint32_t nconst,
                        const uint32_t* program, uint32_t nops, uint64_t n,
                        uint32_t rot_scale, const fp256* y, fp256* d_out);

// gate.hip — pointwise Fr vector op on device buffers (synchronizes).
int fr_vec_op_device(spectre_gpu_ctx* ctx, int dev, int op, const fp256* d_a,
                     const fp256* d_b, const fp256* c, fp256* d_out,
                     uint64_t n);
// gate.hip — out[i] = sum_k coeffs[k] * polys[k][i] over the 1..
// SPECTRE_OPEN_MAX_POLYS device pointers of the host array d_polys
// (synchronizes). d_out may equal any of them.
int fr_lincomb_device(spectre_gpu_ctx* ctx, int dev,
                      const fp256* const* d_polys, const fp256* coeffs,
                      uint32_t m, fp256* d_out, uint64_t n);
// gate.hip — out[i] = a[i] * table[i mod period], table = `period` host
// elements, period a power of two <= SPECTRE_VEC_PERIOD_MAX (synchronizes).
// d_out may alias d_a.
int fr_vec_mul_periodic_device(spectre_gpu_ctx* ctx, int dev,
                               const fp256* d_a, const fp256* table,
                               uint32_t period, fp256* d_out, uint64_t n);
// ntt.hip — the axis log sizes k[0..npass) of a 2^log_n transform, 1 <=
// log_n <= 28 (pure; host). Returns npass.
uint32_t ntt_split(uint32_t log_n, bool force3, uint32_t k[3]);
// ntt.hip — in-place NTT on a device buffer (synchronizes the stream).
int ntt_device(spectre_gpu_ctx* ctx, int dev, fp256* d_data, uint32_t log_n,
               const fp256& omega, int inverse, const fp256* coset_gen);
// ntt.hip — forward (coset) NTT at 2^(log_n + ext_bits) of the 2^log_n
// elements of d_coeffs followed by zeros, into d_out (synchronizes). d_out
// is d_coeffs or does not overlap it; nothing behind the 2^log_n
// coefficients is read. The caller has checked log_n + ext_bits <= 28.
int ntt_extend_device(spectre_gpu_ctx* ctx, int dev, const fp256* d_coeffs,
                      uint32_t log_n, uint32_t ext_bits, fp256* d_out,
                      const fp256& omega_ext, const fp256* coset_gen);

// poly.hip — out[i] = in[i]^-1, zero staying zero (synchronizes). d_out may
// alias d_in.
int fr_batch_invert_device(spectre_gpu_ctx* ctx, int dev, const fp256* d_in,
                           fp256* d_out, uint64_t n);
// poly.hip — z[i] = z0 * prod_{j<i} num[j] * den[j]^-1 (d_den may be null),
// *out_last (may be null) = the i = n value (synchronizes). d_z may alias
// d_num or d_den.
int fr_grand_product_device(spectre_gpu_ctx* ctx, int dev, const fp256* d_num,
                            const fp256* d_den, const fp256& z0, fp256* d_z,
                            uint64_t n, fp256* out_last);
// poly.hip — out[p] = sum_i coeffs[i] * points[p]^i for 1..8 host points,
// one read of d_coeffs (synchronizes). points / out are host memory.
int fr_poly_eval_device(spectre_gpu_ctx* ctx, int dev, const fp256* d_coeffs,
                        uint64_t n, const fp256* points, uint32_t npoints,
                        fp256* out);
// poly.hip — a(X) = (X - z) q(X) + rem: q -> d_q (n elements, q[n-1] = 0),
// *out_rem (may be null) = a(z) (synchronizes). d_q may alias d_a.
int fr_poly_div_linear_device(spectre_gpu_ctx* ctx, int dev, const fp256* d_a,
                              const fp256& z, fp256* d_q, uint64_t n,
                              fp256* out_rem);
// poly.hip — out[k * npoints + p] = sum_i polys[k][i] * points[p]^i for the
// 1..SPECTRE_OPEN_MAX_POLYS device pointers of the host array d_polys and
// 1..8 host points, one read of each polynomial (synchronizes).
int fr_poly_eval_batch_device(spectre_gpu_ctx* ctx, int dev,
                              const fp256* const* d_polys, uint32_t npolys,
                              uint64_t n, const fp256* points,
                              uint32_t npoints, fp256* out);
// poly.hip — fr_poly_div_linear_device by roots[0..nroots) in turn, 1 <=
// nroots <= 8: d_a -> d_q, then in place in d_q; out_rems (may be null) =
// the nroots remainders (synchronizes once). d_q may alias d_a.
int fr_poly_div_roots_device(spectre_gpu_ctx* ctx, int dev, const fp256* d_a,
                             const fp256* roots, uint32_t nroots, fp256* d_q,
                             uint64_t n, fp256* out_rems);
// poly.hip — the built-in tile of the calls above, and whether a
// ctx->fr_scan_tile value is usable (pure; host).
uint32_t fr_scan_tile_default();
bool fr_scan_tile_valid(uint32_t elems);

// lookup.hip — halo2's permute_expression_pair over u <= 2^28 rows: the
// input sorted by canonical value -> d_input_perm, the matching table
// arrangement -> d_table_perm (synchronizes). SPECTRE_ERR_LOOKUP_MISS when
// an input value is not in the table. The four buffers do not overlap.
int fr_lookup_permute_device(spectre_gpu_ctx* ctx, int dev,
                             const fp256* d_input, const fp256* d_table,
                             fp256* d_input_perm, fp256* d_table_perm,
                             uint64_t u);

// perm.hip — out[i] = c * g^i for i < n <= 2^28, any field elements c and g
// (synchronizes).
int fr_powers_device(spectre_gpu_ctx* ctx, int dev, const fp256& c,
                     const fp256& g, fp256* d_out, uint64_t n);
// perm.hip — one chunk of the permutation argument's grand-product terms over
// rows 0..n, n <= 2^28 (synchronizes):
//   den[i] = prod_{j<m} (values[j][i] + beta*sigmas[j][i] + gamma)
//   num[i] = prod_{j<m} (values[j][i] + beta*delta0*delta^j*omega^i + gamma)
// d_values / d_sigmas = host arrays of m device pointers, 1 <= m <=
// SPECTRE_PERM_MAX_COLS. The outputs overlap nothing.
int fr_permutation_terms_device(spectre_gpu_ctx* ctx, int dev,
                                const fp256* const* d_values,
                                const fp256* const* d_sigmas, uint32_t m,
                                const fp256& beta, const fp256& gamma,
                                const fp256& omega, const fp256& delta0,
                                const fp256& delta, fp256* d_num, fp256* d_den,
                                uint64_t n);
