/* spectre_gpu.h — C ABI of the MI355X-native BN254 MSM/NTT proving backend.
 * Besides the two transforms it carries the per-column stages that keep a
 * proof's polynomials on the device between them: gate evaluation and vector
 * ops (quotient phase), batch inverse and grand product (Z columns), the
 * lookup argument's sorted input and permuted table columns, the permutation
 * argument's grand-product terms and row-power columns, and polynomial
 * evaluation and (X - z) division (opening phase), with the set-level forms
 * a multiopen argument loops over: a linear combination of up to 32
 * polynomials, their evaluation at one point set, and division by the set.
 *
 * This is the drop-in boundary for the Spectre/halo2 proving hot path: the
 * reference's own seam is the pair of free functions
 *   best_multiexp(coeffs: &[Fr], bases: &[G1Affine]) -> G1   and
 *   best_fft(a: &mut [Fr], omega: Fr, log_n: u32)
 * in halo2_proofs::arithmetic / halo2curves (reached from every proof and
 * keygen via lightclient-circuits/src/util/circuit.rs:131,158,177,211 in the
 * reference tree). A patched halo2_proofs calls these entry points through a
 * ~100-line unsafe extern "C" block; see INTEGRATION.md for the Rust-side
 * binding a maintainer would add.
 *
 * Data formats (= halo2curves-axiom 0.5.2 memory images, little-endian):
 *   Fr/Fq element : 32 B = 4 x u64 LE limbs of the Montgomery residue
 *                   a*2^256 mod m (the raw &[Fr] slice memory).
 *   canonical Fr  : 32 LE bytes of the integer itself (Fr::to_repr()).
 *   G1 affine     : 64 B = x || y Montgomery Fq; identity = 64 zero bytes.
 *   G1 Jacobian   : 96 B = X || Y || Z Montgomery Fq; identity: Z = 0
 *                   (shard partial sums only; never a caller-visible result).
 *
 * Thread safety: all calls on one ctx are serialized internally; halo2 may
 * invoke commits from concurrent rayon workers. Errors: 0 = ok, negative =
 * failure; spectre_gpu_last_error() returns a thread-local message. The
 * library REQUIRES a visible AMD GPU for every compute entry point (there is
 * deliberately no CPU fallback — a missing GPU fails loudly); the only
 * host-only entry points are spectre_gpu_msm_g1_combine(_windows),
 * spectre_gpu_msm_acc_auto_entries, spectre_gpu_msm_fold_window,
 * spectre_gpu_fr_scan_tile_default, spectre_gpu_ntt_split and the
 * format/version queries.
 */
#ifndef SPECTRE_GPU_H
#define SPECTRE_GPU_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spectre_gpu_ctx spectre_gpu_ctx;

/* scalars argument encoding for MSM entry points */
#define SPECTRE_SCALARS_MONTGOMERY 0u /* raw &[Fr] memory (the real seam) */
#define SPECTRE_SCALARS_CANONICAL 1u  /* already to_repr()'d */

#define SPECTRE_MSM_WINDOW_BITS 16u /* signed window width c */
#define SPECTRE_MSM_NUM_WINDOWS 16u /* ceil(255/c) windows */
#define SPECTRE_MSM_MAX_BATCH 32    /* max scalar vectors per batched call */

/* ctx over `device_count` HIP devices (device_ids NULL -> 0..count-1).
 * Returns NULL on failure (no GPU, bad ids). */
spectre_gpu_ctx* spectre_gpu_init(int device_count, const int* device_ids);
void spectre_gpu_destroy(spectre_gpu_ctx*);
const char* spectre_gpu_last_error(void); /* thread-local, valid until next call */
int spectre_gpu_device_count(spectre_gpu_ctx*);
const char* spectre_gpu_version(void);

/* ---- MSM (host pointers) ------------------------------------------------
 * out_affine = Sum_i scalars[i] * bases[i].  bases_id != 0: the uploaded
 * bases are cached on-device under (bases_id, n) and `bases` may be NULL on
 * subsequent calls (SRS reuse across proofs). num_gpus in [1, device_count]:
 * the scalar/base stream is sharded contiguously, each device runs the full
 * Pippenger pipeline on its shard, partial window sums are combined on host
 * in rank order. */
int spectre_gpu_msm_g1(spectre_gpu_ctx*, uint64_t bases_id,
                       const uint8_t* bases /* n*64B */,
                       const uint8_t* scalars /* n*32B */, uint64_t n,
                       uint32_t flags, int num_gpus, uint8_t out_affine[64]);

/* Batched MSM: `nbatch` scalar vectors (batch-major, nbatch*n*32 B) over ONE
 * shared base set — the shape of create_proof's back-to-back column commits
 * (same SRS); one fused sort/accumulate pass, bases stay cache-resident
 * across the batch. out_affine receives nbatch results (64 B each).
 * nbatch outside 1..SPECTRE_MSM_MAX_BATCH is refused with -3 before anything
 * is sized by it, n == 0 included. */
int spectre_gpu_msm_g1_batch(spectre_gpu_ctx*, uint64_t bases_id,
                             const uint8_t* bases /* n*64B */,
                             const uint8_t* scalars /* nbatch*n*32B */,
                             uint32_t nbatch, uint64_t n, uint32_t flags,
                             uint8_t* out_affine);
int spectre_gpu_msm_g1_batch_device(spectre_gpu_ctx*, int dev,
                                    const void* d_bases,
                                    const void* d_scalars, uint32_t nbatch,
                                    uint64_t n, uint32_t flags,
                                    uint8_t* out_affine);

/* ---- MSM (device-resident, single device `dev`) ------------------------ */
int spectre_gpu_msm_g1_device(spectre_gpu_ctx*, int dev,
                              const void* d_bases, const void* d_scalars,
                              uint64_t n, uint32_t flags,
                              uint8_t out_affine[64]);
/* Per-window Jacobian partial sums of this shard (for cross-process
 * sharding, e.g. one rank per GPU exchanging partials over RCCL):
 * out_partials = SPECTRE_MSM_NUM_WINDOWS * 96 bytes. */
int spectre_gpu_msm_g1_shard_device(spectre_gpu_ctx*, int dev,
                                    const void* d_bases,
                                    const void* d_scalars, uint64_t n,
                                    uint32_t flags, uint8_t* out_partials);
/* As shard_device, plus per-stage timings from HIP events recorded on the
 * library's own stream (the bench's live roofline measurement):
 * out_ms[0..5] = digits, radix-sort, offsets, bucket-accumulate, chunks,
 * reduce-tree; out_ms[6] = total GPU ms; out_ms[7] = count of real
 * (non-zero-digit) sort entries processed. */
int spectre_gpu_msm_g1_shard_device_timed(spectre_gpu_ctx*, int dev,
                                          const void* d_bases,
                                          const void* d_scalars, uint64_t n,
                                          uint32_t flags,
                                          uint8_t* out_partials,
                                          double out_ms[8]);
/* Pipelined (async) shard MSM: enqueue the full pipeline on one of three
 * per-device slots (own stream + scratch) and return WITHOUT synchronizing;
 * *out_slot receives the slot id. Back-to-back MSMs on successive slots
 * overlap call i's latency-bound reduction tail with call i+1's
 * digits/sort/accumulate (create_proof's ~45 commits per proof arrive
 * exactly this way). out_partials (NUM_WINDOWS * 96 B) must stay valid
 * until spectre_gpu_msm_slot_wait(ctx, dev, slot) returns. At most one
 * call may be in flight per slot: a further one fails with -3, and so does
 * a synchronous MSM (they run on slot 0) while slot 0 has one in flight. */
int spectre_gpu_msm_g1_shard_device_async(spectre_gpu_ctx*, int dev,
                                          const void* d_bases,
                                          const void* d_scalars, uint64_t n,
                                          uint32_t flags,
                                          uint8_t* out_partials,
                                          int* out_slot);
int spectre_gpu_msm_slot_wait(spectre_gpu_ctx*, int dev, int slot);
/* Bucket accumulation gives every thread `e` consecutive sorted entries.
 * e = 0 (the default) chooses it per call so that small inputs still put
 * work on every compute unit; any other multiple of 4 up to
 * SPECTRE_MSM_ACC_ENTRIES_MAX fixes it (tests, tuning). The result bytes do
 * not depend on it. Applies to calls enqueued after it returns. */
#define SPECTRE_MSM_ACC_ENTRIES_MAX (1u << 20)
int spectre_gpu_set_msm_acc_entries(spectre_gpu_ctx*, uint32_t e);
/* The auto rule itself (host-only, pure): entries per thread for `entries`
 * sort entries on a device with `cus` compute units that keeps
 * `resident_blocks` accumulate workgroups resident on each. */
uint32_t spectre_gpu_msm_acc_auto_entries(uint64_t entries, uint32_t cus,
                                          uint32_t resident_blocks);
/* The device reduction tail leaves three Jacobian partials per window, and
 * the library folds them on the host before it hands out window sums:
 *   out = p0 + SPECTRE_MSM_TAIL_CHUNK * (p1 + SPECTRE_MSM_TAIL_LO * p2).
 * This is that fold (host-only, pure; 96 B Jacobian each, out may alias an
 * input). Callers of the MSM entry points never see the partials. */
#define SPECTRE_MSM_TAIL_CHUNK 8u /* buckets per chunk of the default build */
#define SPECTRE_MSM_TAIL_LO 64u   /* columns of a window's chunk grid */
int spectre_gpu_msm_fold_window(const uint8_t p0[96], const uint8_t p1[96],
                                const uint8_t p2[96], uint8_t out[96]);
/* Combine gathered shard partials (host-only, deterministic rank order):
 * partials = nshards * NUM_WINDOWS * 96 B. */
int spectre_gpu_msm_g1_combine(const uint8_t* partials, uint32_t nshards,
                               uint8_t out_affine[64]);

/* ---- window-sharded multi-GPU --------------------------------------------
 * Scalar-chunk sharding (above) divides only the bucket work: the
 * per-window reduction tail is fixed per rank, so strong scaling stalls.
 * Window sharding instead gives rank r of R the windows
 * [r*NUM_WINDOWS/R, (r+1)*NUM_WINDOWS/R) over ALL n points: bucket work AND
 * tail divide by R, and the exchange is a pure allgather of DISJOINT window
 * sums (no reduction at all). R must divide NUM_WINDOWS (1,2,4,8,16).
 * out_partials = w_cnt * 96 B Jacobian sums. */
int spectre_gpu_msm_g1_shard_windows_device(spectre_gpu_ctx*, int dev,
                                            const void* d_bases,
                                            const void* d_scalars, uint64_t n,
                                            uint32_t flags, uint32_t w_lo,
                                            uint32_t w_cnt,
                                            uint8_t* out_partials);
/* async variant on the pipeline slots (same contract as
 * spectre_gpu_msm_g1_shard_device_async). */
int spectre_gpu_msm_g1_shard_windows_device_async(
    spectre_gpu_ctx*, int dev, const void* d_bases, const void* d_scalars,
    uint64_t n, uint32_t flags, uint32_t w_lo, uint32_t w_cnt,
    uint8_t* out_partials, int* out_slot);
/* Concatenated rank-ordered slices (nshards * (NUM_WINDOWS/nshards) * 96 B)
 * -> affine result. nshards must divide NUM_WINDOWS. */
int spectre_gpu_msm_g1_combine_windows(const uint8_t* partials,
                                       uint32_t nshards,
                                       uint8_t out_affine[64]);

/* ---- NTT ----------------------------------------------------------------
 * In-place radix-2 NTT over Fr, Montgomery-form data, exactly halo2's
 * best_fft / EvaluationDomain semantics:
 *   if coset_gen && !inverse : data[i] *= coset_gen^i            (before)
 *   data <- DFT(data, omega)     [caller passes omega_inv to invert]
 *   if inverse               : data[i] *= n^{-1}
 *   if coset_gen && inverse  : data[i] *= coset_gen^i   (after; pass g^{-1})
 * log_n <= 28 (= BN254 Fr's 2-adicity; the reference needs 2^20..2^24 for
 * its circuits and 2^25..2^26 extended domains for aggregation). */
int spectre_gpu_ntt_fr(spectre_gpu_ctx*, uint8_t* data, uint32_t log_n,
                       const uint8_t omega[32], int inverse,
                       const uint8_t* coset_gen);
int spectre_gpu_ntt_fr_device(spectre_gpu_ctx*, int dev, void* d_data,
                              uint32_t log_n, const uint8_t omega[32],
                              int inverse, const uint8_t* coset_gen);
/* The rule that splits a 2^log_n transform into passes (host-only, pure;
 * tests): k[0 .. count) receive the axis log sizes in pass order, each in
 * 1..12 and summing to log_n, the rest of k is zeroed, and the pass count
 * (1..3) is returned. force3 != 0 is the rule a context created under
 * SPECTRE_NTT_FORCE3 follows. Returns 0 for log_n == 0 or log_n > 28. */
uint32_t spectre_gpu_ntt_split(uint32_t log_n, int force3, uint32_t k[3]);
/* out[t] = sum_{i < n} a[i] * coset_gen^i * omega_ext^(i*t),  t < N,
 * n = 2^log_n, N = 2^(log_n + ext_bits): halo2's coeff_to_extended
 * (distribute_powers_zeta, resize with zeros, best_fft at extended_k).
 * d_coeffs: n elements, d_out: N elements, device `dev`, Montgomery Fr.
 * coset_gen NULL: no coset factor. ext_bits = 0 is the plain forward
 * (coset) NTT out of place. log_n + ext_bits <= 28.
 * d_out == d_coeffs is allowed (a buffer of N elements whose first n hold
 * the coefficients); its other N - n elements are NEVER READ and need not be
 * initialised. Otherwise the two ranges must not overlap, and d_coeffs is
 * not written. Synchronizes. */
int spectre_gpu_ntt_fr_extend_device(spectre_gpu_ctx*, int dev,
                                     const void* d_coeffs, uint32_t log_n,
                                     uint32_t ext_bits, void* d_out,
                                     const uint8_t omega_ext[32],
                                     const uint8_t* coset_gen);

/* ---- pointwise Fr vector ops (device buffers, Montgomery form) ----------
 * The quotient phase evaluates gate expressions pointwise between the
 * iFFT and coset-FFT passes; these ops let a patched evaluator keep
 * polynomials device-resident. out may alias a or b, and
 * a may alias b, where "alias" means the SAME pointer: a lane reads element
 * i of its inputs before it writes element i and touches no other. Buffers
 * that overlap without being equal are not supported (and not checked).
 *   op 0: out = a + b        op 1: out = a - b       op 2: out = a * b
 *   op 3: out = a * c        op 4: out = a + c * b   (c = one Fr element)
 * Refused with -1: op outside 0..4, NULL d_a or d_out, NULL d_b for ops
 * 0, 1, 2 and 4, NULL c for ops 3 and 4. n == 0: nothing is done and 0 is
 * returned. Synchronizes.
 */
/* ---- gate-expression evaluator (quotient phase) -------------------------
 * Evaluates one custom-gate expression over every row of a (usually
 * extended-domain) column set in a single launch — the device-resident
 * iFFT -> gate-eval -> coset-FFT quotient pipeline needs O(1) launches per
 * gate instead of per-op round trips.
 *
 * program = nops * 3 uint32 words {op, a, b}, a stack machine:
 *   COL   a=column index, b=(int32) rotation: push cols[a][(row + b*rot_scale) mod n]
 *   CONST a=constant index: push constants[a]  (challenges, coefficients)
 *   ADD/SUB/MUL: pop two (second-from-top OP top), push result
 *   NEG: negate top
 * Stack depth is validated <= SPECTRE_GATE_MAX_DEPTH. All values are
 * Montgomery Fr (32 B LE). On exit, for each row:
 *   y == NULL : out[row]  = result               (first gate)
 *   y != NULL : out[row] = out[row]*y + result   (halo2's h = h*y + gate)
 * d_cols is a HOST array of ncols DEVICE pointers; constants/program/y are
 * host pointers. n is a nonzero power of two.
 *
 * Refused before anything is launched, and then nothing is written:
 *   -1  a NULL d_cols, program or d_out, nops == 0, NULL constants with
 *       nconst != 0; a NULL entry in d_cols, whether or not the program
 *       reads that column; any byte shared between d_out[0..n) and any
 *       d_cols[j][0..n), equal pointers included (a lane reads rotated rows
 *       that other lanes write, so no overlap has a defined result);
 *   -3  n zero or not a power of two; a malformed program (unknown opcode,
 *       column index >= ncols, constant index >= nconst, an operator on too
 *       short a stack, depth above SPECTRE_GATE_MAX_DEPTH, a final stack of
 *       other than one value); a rotation with |b * rot_scale| >= n, the
 *       product taken in 64 bits (rot_scale == 0 makes every rotation 0). */
#define SPECTRE_GATE_OP_COL 0
#define SPECTRE_GATE_OP_CONST 1
#define SPECTRE_GATE_OP_ADD 2
#define SPECTRE_GATE_OP_SUB 3
#define SPECTRE_GATE_OP_MUL 4
#define SPECTRE_GATE_OP_NEG 5
#define SPECTRE_GATE_MAX_DEPTH 8
int spectre_gpu_fr_gate_eval(spectre_gpu_ctx*, int dev,
                             const void* const* d_cols, uint32_t ncols,
                             const uint8_t* constants, uint32_t nconst,
                             const uint32_t* program, uint32_t nops,
                             uint64_t n, uint32_t rot_scale,
                             const uint8_t* y /* 32 B or NULL */,
                             void* d_out);

#define SPECTRE_VEC_ADD 0
#define SPECTRE_VEC_SUB 1
#define SPECTRE_VEC_MUL 2
#define SPECTRE_VEC_SCALE 3
#define SPECTRE_VEC_ADD_SCALED 4
int spectre_gpu_fr_vec_op(spectre_gpu_ctx*, int dev, int op,
                          const void* d_a, const void* d_b /* NULL for op 3 */,
                          const uint8_t c[32] /* NULL for ops 0-2 */,
                          void* d_out, uint64_t n);
/* out[i] = a[i] * table[i mod period] — halo2's divide_by_vanishing_poly
 * with table = t_evaluations. table: host, period*32 B, Montgomery Fr;
 * period a power of two, 1 <= period <= SPECTRE_VEC_PERIOD_MAX (64).
 * d_out may alias d_a. n == 0: nothing is done. Synchronizes. */
#define SPECTRE_VEC_PERIOD_MAX 64u
int spectre_gpu_fr_vec_mul_periodic(spectre_gpu_ctx*, int dev, const void* d_a,
                                    const uint8_t* table, uint32_t period,
                                    void* d_out, uint64_t n);

/* ---- grand products (device buffers, Montgomery Fr) ---------------------
 * The permutation and lookup arguments build, per column,
 *   Z[0] = 1 (or the previous chunk's last value), Z[i+1] = Z[i]*num[i]/den[i]
 * which halo2 computes with batch_invert, a pointwise multiply and a serial
 * running product. These two calls keep that stage on the device. All
 * buffers are device pointers on device `dev`; the calls synchronize. */
/* out[i] = in[i]^-1; a zero element stays zero (ff::BatchInvert / halo2
 * batch_invert semantics). d_out may alias d_in. */
int spectre_gpu_fr_batch_invert(spectre_gpu_ctx*, int dev, const void* d_in,
                                void* d_out, uint64_t n);
/* z[0] = z0, z[i] = z0 * prod_{j<i} num[j] * den[j]^-1   for i < n;
 * out_last = z0 * prod_{j<n} ...  (the value halo2 carries into the next
 * permutation chunk). d_den == NULL: no denominators. z0 == NULL: one.
 * out_last may be NULL. A zero denominator inverts to zero (as above), so
 * every later z is zero. d_z may alias d_num or d_den. n <= 2^28. */
int spectre_gpu_fr_grand_product(spectre_gpu_ctx*, int dev, const void* d_num,
                                 const void* d_den, const uint8_t z0[32],
                                 void* d_z, uint64_t n, uint8_t out_last[32]);
/* Elements per workgroup tile of the two kernels above. 0 (default) = the
 * built-in choice; otherwise a multiple of the block size (256) up to the
 * default (tests, tuning). Result bytes do not depend on it. */
int spectre_gpu_set_fr_scan_tile(spectre_gpu_ctx*, uint32_t elems);
uint32_t spectre_gpu_fr_scan_tile_default(void); /* host-only, pure */

/* ---- opening phase (device buffers, Montgomery Fr) -----------------------
 * Between the last challenge and the two multiopen commits halo2 evaluates
 * every queried coefficient-form polynomial at x*omega^rot
 * (eval_polynomial) and divides by (X - z) per opening point
 * (kate_division). These two calls do both on the buffers the inverse NTT
 * left on device `dev`, so no polynomial is downloaded; the calls
 * synchronize. Points, z and results are host memory. The workgroup tile is
 * the one spectre_gpu_set_fr_scan_tile sets; result bytes do not depend on
 * it. */
#define SPECTRE_POLY_EVAL_MAX_POINTS 8u
/* out[p] = sum_{i<n} a[i] * points[p]^i for p < npoints, one read of a.
 * d_coeffs: device, n elements. points/out: host, npoints*32 B.
 * n == 0: every out[p] = 0. 1 <= npoints <= MAX_POINTS. n <= 2^28. */
int spectre_gpu_fr_poly_eval(spectre_gpu_ctx*, int dev, const void* d_coeffs,
                             uint64_t n, const uint8_t* points,
                             uint32_t npoints, uint8_t* out);
/* a(X) = (X - z) * q(X) + rem:
 *   q[i] = sum_{j=i+1}^{n-1} a[j] * z^(j-i-1)  for i < n   (so q[n-1] = 0)
 *   rem  = a(z)
 * q[0 .. n-1) is exactly halo2's kate_division(a, z). d_q has n elements
 * and may alias d_a. out_rem may be NULL. n == 0: rem = 0, nothing is
 * written. No inverse of z is taken: z = 0 and z = 1 are ordinary inputs.
 * n <= 2^28. */
int spectre_gpu_fr_poly_div_linear(spectre_gpu_ctx*, int dev, const void* d_a,
                                   const uint8_t z[32], void* d_q, uint64_t n,
                                   uint8_t out_rem[32]);

/* The set-level forms of the two calls above and of the ADD_SCALED chain
 * around them: what SHPLONK / GWC do per rotation set in one call each.
 * Serialized and synchronizing like their neighbours; a rejected call writes
 * nothing. Both batched calls take at most SPECTRE_OPEN_MAX_POLYS
 * polynomials; a longer sum is chained through the accumulator (below). */
#define SPECTRE_OPEN_MAX_POLYS 32u
/* out[i] = sum_{k<m} coeffs[k] * polys[k][i]   for i < n.
 * d_polys: HOST array of m DEVICE pointers, n elements each. coeffs: host,
 * m*32 B. 1 <= m <= MAX_POLYS, n <= 2^28; n == 0 does nothing. d_out may
 * EQUAL any of the inputs and one pointer may be listed several times: to
 * accumulate, or to chain past MAX_POLYS, list the accumulator with
 * coefficient one. Any other overlap of d_out with an input is refused, as
 * is a NULL entry. Exactly n elements are written; inputs are never written.
 * The sum is exact, so the bytes are those of halo2's Horner in y. */
int spectre_gpu_fr_lincomb(spectre_gpu_ctx*, int dev,
                           const void* const* d_polys, const uint8_t* coeffs,
                           uint32_t m, void* d_out, uint64_t n);
/* out[k*npoints + p] = sum_{i<n} polys[k][i] * points[p]^i: every polynomial
 * of a rotation set at the set's points, one read of each polynomial and one
 * synchronization. d_polys: HOST array of m DEVICE pointers, n elements
 * each; one pointer may be listed twice. points: host, npoints*32 B. out:
 * host, m*npoints*32 B. 1 <= m <= MAX_POLYS, 1 <= npoints <=
 * SPECTRE_POLY_EVAL_MAX_POINTS, n <= 2^28; n == 0: every output is zero.
 * Inputs are never written. */
int spectre_gpu_fr_poly_eval_batch(spectre_gpu_ctx*, int dev,
                                   const void* const* d_polys, uint32_t m,
                                   uint64_t n, const uint8_t* points,
                                   uint32_t npoints, uint8_t* out);
/* spectre_gpu_fr_poly_div_linear applied nroots times, in the order of
 * `roots`, with one synchronization: the first division goes d_a -> d_q, the
 * rest run in place in d_q; out_rems[j] is the remainder of division j.
 * roots: host, nroots*32 B. out_rems: host, nroots*32 B, or NULL.
 * 1 <= nroots <= 8, n <= 2^28. d_q may equal d_a (any other overlap is
 * refused); out of place d_a is not written. n == 0: the remainders are
 * zero and nothing is written. No inverse is taken: repeated roots, 0 and 1
 * are ordinary inputs. What follows from the definition, with
 * Z_S = prod_j (X - roots[j]):
 *   quotient    q is the quotient of a by Z_S; the top min(nroots, n)
 *               elements of d_q are zero.
 *   remainders  they are the Newton coefficients of the remainder:
 *                 a = Z_S * q + sum_j rems[j] * prod_{i<j} (X - roots[i])
 *   no r_i      a multiopen prover need not subtract the interpolant r_i of
 *               f_i's evaluations over S before dividing: the quotient of
 *               f_i by Z_S already is (f_i - r_i) / Z_S.
 *   a check     out_rems is r_i in Newton form over the roots in order, so
 *               the caller can assert it against its own interpolation. */
int spectre_gpu_fr_poly_div_roots(spectre_gpu_ctx*, int dev, const void* d_a,
                                  const uint8_t* roots, uint32_t nroots,
                                  void* d_q, uint64_t n, uint8_t* out_rems);

/* ---- lookup argument (device buffers, Montgomery Fr) ---------------------
 * halo2's permute_expression_pair over the u usable rows of a lookup's
 * compressed input column A and table column S (u = n - blinding_factors -
 * 1; the caller fills the blinding rows afterwards, as it does today).
 * A' = A[0..u) sorted by canonical value; S' as halo2's
 * permute_expression_pair builds it. Montgomery Fr, device buffers on `dev`;
 * exactly u elements of each output are written. The four buffers must not
 * overlap. u == 0: nothing is written. u <= 2^28. Synchronizes.
 * Every row then has A'[i] == S'[i] or A'[i] == A'[i-1]. The order is
 * Fr::cmp's, of the integer a and not of its Montgomery image; elements are
 * reduced residues. An input value that the table does not hold fails the
 * call with SPECTRE_ERR_LOOKUP_MISS (halo2: Error::ConstraintSystemFailure);
 * spectre_gpu_last_error() then gives the number of distinct input values
 * that were missing, and the output contents are unspecified. The inputs
 * are never written. */
#define SPECTRE_ERR_LOOKUP_MISS (-5)
int spectre_gpu_fr_lookup_permute(spectre_gpu_ctx*, int dev,
                                  const void* d_input, const void* d_table,
                                  void* d_input_perm, void* d_table_perm,
                                  uint64_t u);

/* ---- permutation argument (device buffers, Montgomery Fr) ----------------
 * halo2's permutation::prover::commit builds each Z column from per-row
 * products that need omega^i, and the extended-domain permutation constraint
 * needs X_i = zeta * omega_ext^i. These two calls make both on device `dev`;
 * they synchronize. A permutation Z column is then
 *   permutation_terms -> fr_grand_product(num, den, z0 = the previous
 *   chunk's out_last) over the usable rows,
 * chunks chaining through out_last and delta0 <- delta0 * delta^m; the
 * constraint is an fr_gate_eval program over one extra column,
 * fr_powers(zeta, omega_ext, 2^extended_k), built once per domain. */
/* out[i] = c * g^i, i < n.  c == NULL: one.  g, c: host, 32 B Montgomery Fr,
 * any field elements (g need not be a root of unity; g = 0 gives c,0,0,...).
 * n == 0: nothing is done. n <= 2^28. */
int spectre_gpu_fr_powers(spectre_gpu_ctx*, int dev, const uint8_t c[32],
                          const uint8_t g[32], void* d_out, uint64_t n);

#define SPECTRE_PERM_MAX_COLS 8u
/* One chunk of halo2's permutation::prover::commit, rows 0..n:
 *   den[i] = prod_{j<m} (values[j][i] + beta*sigmas[j][i]          + gamma)
 *   num[i] = prod_{j<m} (values[j][i] + beta*delta0*delta^j*omega^i + gamma)
 * d_values, d_sigmas: HOST arrays of m DEVICE pointers (n elements each);
 * 1 <= m <= SPECTRE_PERM_MAX_COLS. delta0 = delta^(index of the chunk's first
 * column), the value halo2 carries from chunk to chunk; NULL: one.
 * d_num, d_den: n elements each. They must not overlap each other or any
 * input. Exactly n elements of each are written; inputs are never written.
 * n is any row count <= 2^28 (the caller passes the usable rows or the
 * whole column). n == 0: nothing is done. */
int spectre_gpu_fr_permutation_terms(spectre_gpu_ctx*, int dev,
        const void* const* d_values, const void* const* d_sigmas, uint32_t m,
        const uint8_t beta[32], const uint8_t gamma[32],
        const uint8_t omega[32], const uint8_t delta0[32],
        const uint8_t delta[32], void* d_num, void* d_den, uint64_t n);

/* ---- device memory helpers (for C callers and the bench harness) ------- */
int spectre_gpu_malloc(spectre_gpu_ctx*, int dev, size_t bytes, void** d_ptr);
int spectre_gpu_free(spectre_gpu_ctx*, int dev, void* d_ptr);
int spectre_gpu_upload(spectre_gpu_ctx*, int dev, void* d_dst, const void* src,
                       size_t bytes);
int spectre_gpu_download(spectre_gpu_ctx*, int dev, void* dst,
                         const void* d_src, size_t bytes);
int spectre_gpu_synchronize(spectre_gpu_ctx*, int dev);

#ifdef __cplusplus
}
#endif
#endif /* SPECTRE_GPU_H */
