// ntt.hip — radix-2 NTT over BN254 Fr for gfx950 (MI355X).
//
// Computes what halo2's best_fft / EvaluationDomain compute (the plain DFT
// out[j] = Sum_i a[i] omega^(ij); inverse = DFT with omega^{-1} then * n^{-1};
// coset = multiply by coset_gen^i before (forward) / after (inverse)).
//
// MI355X-native structure (four-step / Bailey decomposition): n = 2^log_n is
// split into one, two or three axes of at most 2^12 elements (ntt_split), so
// each sub-transform fits LDS and the whole transform is one global PASS per
// axis instead of log2(n) of them — with two axes the difference between
// ~1 GiB and ~11.5 GiB of HBM traffic at n=2^23, SURVEY.md §8d. Three axes
// cover log_n in [25, 28] (the aggregation circuits' extended domains reach
// 2^25..2^26; Fr's 2-adicity caps at 2^28).
//
// A pass (k_ntt_pass) transforms one axis of length L = 2^k[p], whose
// elements lie S = 2^(sum of the later axes' k) apart; one workgroup per
// tile m:
//   1. load in[base + s*S] into LDS (the first pass of a forward coset
//      multiplies by g^(global index) on the way in);
//   2. in-LDS DIF; its bit-reversed output order is folded into the store
//      index, costing nothing extra;
//   3. every pass but the last multiplies by the inter-pass twiddle and
//      stores in place, out[base + t*S]; the last pass (S = 1, contiguous
//      coalesced loads) applies n^{-1} and the inverse-coset factor and
//      scatters to the digit-reversed position, which is the natural-order
//      output index.
// Derivation for three axes (i = a*BC + b*C + c, t = tA + A*tB + AB*tC):
//   i*t mod n = a*BC*tA + b*C*(tA + A*tB) + c*(tA + A*tB + AB*tC)
// so pass 1 (axis a, root w^(BC), tile m = b*C + c) is followed by the
// twiddle w^(tA*m); pass 2 (axis b, root w^(AC), m = tA*C + c) by
// w^(A*tB*c) = w^((t << kA) * (m & (C-1))); pass 3 (axis c, root w^(AB),
// m = tA*B + tB) stores to out[tA + A*tB + AB*t]. In general the twiddle
// after a pass is w^((t << sum of the earlier axes' k) * (m & (S-1))). Two
// axes are the case B = 1, one axis A = B = 1. All exponents < n <= 2^28.
// Twiddle/coset powers g^e resolve via the two-level table of powtab.hpp (one
// mul + two cached loads), the omega one built once per (omega, log_n) plan
// and cached on device, the coset one per call.
//
// The extend transform (halo2's coeff_to_extended: 2^k coefficients, zeros up
// to 2^(k+e), coset NTT there) is the same plan and pass loop at 2^(k+e) with
// another first pass, the EXT instantiation of k_ntt_pass: it loads only the
// coefficients and writes the result of the DIF levels that a zero operand
// turns into a copy and one multiply (DESIGN.md "Extended domain").
//
// All Fr math is 8x32-limb Montgomery (ff.hpp); data stays in Montgomery form
// end-to-end exactly as halo2 holds its &[Fr] slices.
//
// This file computes in NttFr, Fr with the C CIOS multiply: the asm column
// multiply regressed the 1024-thread LDS kernels ~7% (2^23 fwd 2.59 -> 2.77
// ms — register pressure at the 4-waves/SIMD occupancy these kernels need),
// while it wins ~28% in the 256-thread MSM kernels. Measured r2.
#include "internal.hpp"
#include <type_traits>

#ifdef SPECTRE_NTT_ASMMUL  // variant: re-tests the asm multiply under new
using NttFr = Fr;          // block geometries
#else
using NttFr = FrCios;
#endif

#define NTT_THREADS 1024  // NTT passes: 16 waves/block so one LDS-resident
                          // block still puts 4 waves on every SIMD

__device__ __forceinline__ uint32_t bitrev(uint32_t x, uint32_t bits) {
    return bits ? (__brev(x) >> (32 - bits)) : 0;
}
// LDS layout: a 32-B element spans 8 banks, so a 16-lane ds_read_b128 group
// covers only 8 bank-octets — inherent 2-8x conflict at power-of-two
// butterfly strides (measured SQ_LDS_BANK_CONFLICT/IDX_ACTIVE = 0.85 with a
// single fp256 array). Instead each element is stored as TWO 16-B halves in
// separate regions (lo at [i], hi at [H+i]; lds_split_ld / lds_split_st):
// consecutive elements stride 4 banks and one lane group covers all 64 banks.
#define LDS_BYTES(L) ((uint32_t)(L) * 32u)

// in-LDS DIF butterflies over L = 2^logL elements; twL[j] = (root)^j, j < L/2.
// On exit lds[s] holds DFT output index bitrev(s, logL).
//
// Levels run in FUSED PAIRS (radix-4 rounds): a thread loads the quad
// (i0, i0+h/2, i0+h, i0+3h/2), applies level h then level h/2 in registers,
// and writes back once — HALF the LDS round trips and HALF the barriers of
// per-level radix-2, with the exact same field operations (bit-identical
// results; finite-field ops are exact). An odd level count runs one plain
// radix-2 level first.
// R4 is a compile-time variant: the radix-4 quad path costs VGPRs/code even
// when branched over at run time (measured 2^20 0.40 -> 0.46 ms with a
// run-time flag), so the host launches the <true> instantiation only when
// the tile gives every thread a quad (L >= 4*threads).
// SKIP (compile-time, the extend pass): the levels h = L/2 .. L >> skip are
// already done, the load phase wrote their result; the remaining logL - skip
// levels keep their twiddle strides, and their parity decides the lone
// radix-2 level. Without SKIP, skip is not looked at.
template <bool R4, bool SKIP>
__device__ void lds_dif(uint4* lds4, uint32_t H, const fp256* __restrict__ twL,
                        uint32_t logL, uint32_t skip) {
    const uint32_t L = 1u << logL;
    const uint32_t levels = SKIP ? logL - skip : logL;
    uint32_t h = SKIP ? (L >> 1) >> skip : L >> 1;
    if (!R4 || (levels & 1))  // radix-2: all levels, or one to make pairs even
    {
        for (; h >= 1; h >>= 1) {
            const uint32_t stride = (L >> 1) / h;
            for (uint32_t p = threadIdx.x; p < (L >> 1); p += blockDim.x) {
                uint32_t blk = p / h, j = p % h;
                uint32_t i0 = blk * 2 * h + j, i1 = i0 + h;
                fp256 u, v, t, w;
                lds_split_ld(lds4, i0, H, u);
                lds_split_ld(lds4, i1, H, v);
                ff_add<NttFr>(w, u, v);
                lds_split_st(lds4, i0, H, w);
                ff_sub<NttFr>(t, u, v);
                ff_mul<NttFr>(t, t, twL[(uint64_t)j * stride]);
                lds_split_st(lds4, i1, H, t);
            }
            __syncthreads();
            if constexpr (R4) { h >>= 1; break; }
        }
    }
    if constexpr (!R4) return;
    for (; h >= 2; h >>= 2) {
        const uint32_t hh = h >> 1;               // second level of the pair
        const uint32_t s_h = (L >> 1) / h;        // level-h twiddle stride
        for (uint32_t p = threadIdx.x; p < (L >> 2); p += blockDim.x) {
            const uint32_t blk = p / hh, j = p % hh;
            const uint32_t i0 = blk * 2 * h + j;
            fp256 a, b, c, d, t;
            lds_split_ld(lds4, i0, H, a);
            lds_split_ld(lds4, i0 + hh, H, b);
            lds_split_ld(lds4, i0 + h, H, c);
            lds_split_ld(lds4, i0 + h + hh, H, d);
            // level h: pairs (a,c) at offset j and (b,d) at offset j+hh
            fp256 a1, b1, c1, d1;
            ff_add<NttFr>(a1, a, c);
            ff_sub<NttFr>(t, a, c);
            ff_mul<NttFr>(c1, t, twL[(uint64_t)j * s_h]);
            ff_add<NttFr>(b1, b, d);
            ff_sub<NttFr>(t, b, d);
            ff_mul<NttFr>(d1, t, twL[(uint64_t)(j + hh) * s_h]);
            // level h/2: pairs (a1,b1) and (c1,d1), both at offset j,
            // twiddle stride 2*s_h
            ff_add<NttFr>(a, a1, b1);
            ff_sub<NttFr>(t, a1, b1);
            ff_mul<NttFr>(b, t, twL[(uint64_t)j * 2 * s_h]);
            ff_add<NttFr>(c, c1, d1);
            ff_sub<NttFr>(t, c1, d1);
            ff_mul<NttFr>(d, t, twL[(uint64_t)j * 2 * s_h]);
            lds_split_st(lds4, i0, H, a);
            lds_split_st(lds4, i0 + hh, H, b);
            lds_split_st(lds4, i0 + h, H, c);
            lds_split_st(lds4, i0 + h + hh, H, d);
        }
        __syncthreads();
    }
}

// One pass: the DFT of tile m (grid.x) of length L = 2^logL at stride
// S = 2^logS, whose element j sits at base + j*S with
//   base = (m >> logS)*L*S + (m & (S-1)).
struct NttPass {
    const fp256* in;
    fp256* out;
    const fp256* twL;        // (axis root)^j, j < L/2
    PowTable omega;          // omega powers (passes before the last)
    PowTable coset;          // coset powers; null T1 = no coset multiply in
                             // this pass (forward: on load, inverse: on the
                             // last pass's store)
    fp256 scale;             // n^{-1}, applied by the last pass of an inverse
    uint32_t logL, logS;
    uint32_t tw_shift;       // sum of the earlier axes' log sizes
    uint32_t fin_logA, fin_logB;  // last pass: m = tA << fin_logB | tB
    uint32_t last, inverse;
};
// The first pass of an extend transform (EXT instantiations only, so the
// plain instantiations keep the parent's kernel arguments): the input holds
// 2^log_in elements and stands for 2^log_in coefficients followed by zeros.
struct NttExtPass : NttPass {
    uint32_t log_in;
    uint32_t prune;  // min(ext_bits, logL): DIF levels done by the load phase
};

// in and out are the same buffer in a middle pass and in a single pass (hence
// no __restrict__): a workgroup has its whole tile in LDS before it stores,
// an in-place pass stores to the positions it loaded, and the last pass's
// scatter runs in place only when its one workgroup is the whole transform.
//
// EXT (compile-time, like R4: the plain instantiations must not pay for it)
// is the first pass of an extend transform. Its input is 2^log_in elements
// long and every index from there up counts as zero, so
//   - in[pos] is loaded only where pos < 2^log_in: nothing behind the
//     coefficients is ever read, which is all that correctness needs at any
//     split, and what lets out alias in with an uninitialised tail;
//   - tile elements s >= L' = L >> prune are zero, so each of the first
//     `prune` DIF levels is a copy and one multiply: after them, block q
//     (q < 2^prune) of the tile holds x[j] * root^(j * bitrev(q, prune)) at
//     offset j < L'. The load phase writes that directly (root^e from twL,
//     root^(L/2) = -1) and the butterflies start at level h = L'/2.
template <bool R4, bool EXT = false>
__global__ __launch_bounds__(NTT_THREADS) void k_ntt_pass(
    std::conditional_t<EXT, NttExtPass, NttPass> p) {
    extern __shared__ uint4 lds4[];
    const uint32_t L = 1u << p.logL;
    const uint32_t H = L;
    const uint32_t m = blockIdx.x;
    const uint32_t mS = m & ((1u << p.logS) - 1);
    const uint64_t base = ((uint64_t)(m >> p.logS) << (p.logL + p.logS)) + mS;
    uint32_t skip = 0;
    if constexpr (EXT) {
        skip = p.prune;
        const uint32_t Lp = L >> skip, half = L >> 1;
        const uint64_t n_in = 1ull << p.log_in;
        for (uint32_t s = threadIdx.x; s < Lp; s += blockDim.x) {
            const uint64_t pos = base + ((uint64_t)s << p.logS);
            fp256 v;
            ff_set_zero(v);
            if (pos < n_in) {
                v = p.in[pos];
                if (p.coset.T1) {  // forward coset: g^(original index)
                    fp256 f;
                    pow_lookup<NttFr>(f, p.coset, (uint32_t)pos);
                    ff_mul<NttFr>(v, v, f);
                }
            }
            lds_split_st(lds4, s, H, v);
            for (uint32_t q = 1; q < (1u << skip); q++) {
                const uint32_t e = s * bitrev(q, skip);  // < L
                fp256 t;
                ff_mul<NttFr>(t, v, p.twL[e & (half - 1)]);
                if (e & half) ff_neg<NttFr>(t, t);
                lds_split_st(lds4, q * Lp + s, H, t);
            }
        }
    } else {
        for (uint32_t s = threadIdx.x; s < L; s += blockDim.x) {
            const uint64_t pos = base + ((uint64_t)s << p.logS);
            fp256 v = p.in[pos];
            if (p.coset.T1 && !p.inverse) {  // forward coset: g^(input index)
                fp256 f;
                pow_lookup<NttFr>(f, p.coset, (uint32_t)pos);
                ff_mul<NttFr>(v, v, f);
            }
            lds_split_st(lds4, s, H, v);
        }
    }
    __syncthreads();
    lds_dif<R4, EXT>(lds4, H, p.twL, p.logL, skip);
    for (uint32_t s = threadIdx.x; s < L; s += blockDim.x) {
        const uint32_t t = bitrev(s, p.logL);
        fp256 v, f;
        lds_split_ld(lds4, s, H, v);
        uint64_t opos;
        if (!p.last) {
            pow_lookup<NttFr>(f, p.omega, (t << p.tw_shift) * mS);
            ff_mul<NttFr>(v, v, f);
            opos = base + ((uint64_t)t << p.logS);
        } else {
            if (p.inverse) ff_mul<NttFr>(v, v, p.scale);
            const uint32_t tA = m >> p.fin_logB;
            const uint32_t tB = m & ((1u << p.fin_logB) - 1);
            opos = (uint64_t)tA + ((uint64_t)tB << p.fin_logA) +
                   ((uint64_t)t << (p.fin_logA + p.fin_logB));
            if (p.coset.T1 && p.inverse) {  // inverse coset: g^(output index)
                pow_lookup<NttFr>(f, p.coset, (uint32_t)opos);
                ff_mul<NttFr>(v, v, f);
            }
        }
        p.out[opos] = v;
    }
}

// ---------------------------------------------------------------- host side
// Axis log sizes k[0..npass) for n = 2^log_n (log_n >= 1), each <= 12; the
// last axis is the contiguous one. Returns npass. force3 takes the three-axis
// rule at sizes that do not need it (testing). Pure; exported as
// spectre_gpu_ntt_split so that tests can pin the rule.
uint32_t ntt_split(uint32_t log_n, bool force3, uint32_t k[3]) {
    if (log_n > 24 || (force3 && log_n >= 3)) {
        // k[0] = 12 gives the first pass 4096-element tiles (radix-4
        // rounds): measured -6% at 2^26 against the balanced split, neutral
        // at 2^25, so from 26 up.
        if (log_n >= 26) {
            k[0] = 12;
            k[1] = (log_n - 12 + 1) / 2;
            k[2] = log_n - 12 - k[1];
        } else {
            const uint32_t q = log_n / 3, r = log_n % 3;
            k[0] = q + (r > 0);
            k[1] = q + (r > 1);
            k[2] = q;
        }
        return 3;
    }
    if (log_n <= 12) {
        k[0] = log_n;
        return 1;
    }
    // Two axes, k[1] >= k[0] (the contiguous pass gets the bigger tile).
    // Measured on MI355X: k[1] = 12 (4096-element tiles -> radix-4 rounds)
    // wins for log_n <= 20 (2^20 fwd 0.40 -> 0.32 ms) but LOSES at 2^22
    // ((10,12) 1.40 vs balanced (11,11) 1.31 ms — the strided pass's longer
    // stride outweighs the contiguous pass's gain), so: 12 up to log_n 20,
    // balanced above (log_n 23/24 balance to 12 anyway).
    k[1] = log_n <= 20 ? 12 : (log_n + 1) / 2;
    k[0] = log_n - k[1];
    return 2;
}

// choose the split and build the twiddle tables for (omega, log_n) into p
static int build_plan(DeviceState& ds, const fp256& omega, uint32_t log_n,
                      bool force3, NttPlan& p) {
    p.npass = ntt_split(log_n, force3, p.k);
    RC_TRY(p.twB.reserve(pow_table_elems(1u << log_n)));
    p.omega = pow_tables_build(ds, omega, nullptr, 1u << log_n, p.twB.ptr);
    for (uint32_t i = 0; i < p.npass; i++) {
        fp256 root;  // of axis i's DFT
        ff_pow_u32<NttFr>(root, omega, 1u << (log_n - p.k[i]));
        const uint32_t half = 1u << (p.k[i] - 1);
        RC_TRY(p.tw[i].reserve(half));
        pow_linear_build(ds, root, p.tw[i].ptr, half);
    }
    return call_finish(ds);
}

// build-or-get the cached twiddle plan for (omega, log_n)
static int get_plan(DeviceState& ds, const fp256& omega, uint32_t log_n,
                    bool force3, NttPlan** out) {
    std::array<uint8_t, 40> key{};
    memcpy(key.data(), omega.l, 32);
    memcpy(key.data() + 32, &log_n, 4);
    auto it = ds.plans.find(key);
    if (it == ds.plans.end()) {
        NttPlan p;  // cached only once complete; a failed build frees it
        const int rc = build_plan(ds, omega, log_n, force3, p);
        if (rc) {
            p.release();
            return rc;
        }
        it = ds.plans.emplace(key, p).first;
    }
    *out = &it->second;
    return 0;
}

// Launch one pass of a 2^log_n transform, one workgroup per tile.
// Thread count: L/4 (radix-4 butterflies occupy exactly L/4 threads; smaller
// blocks co-reside per CU, LDS permitting, keeping occupancy), floored at 128
// for tiny tiles where 64-thread blocks underutilize. Measured against L/1
// and L/2: 2^22 coset 1.45 -> 1.19 ms, 2^23 fwd 2.54 -> 2.26, 2^24
// unchanged, 2^20 within 4% of its best.
// ext_bits < 0: a plain pass. Otherwise the first pass of an extend transform
// whose input is 2^(log_n - ext_bits) elements long.
static void launch_pass(hipStream_t st, const NttPass& pass, uint32_t log_n,
                        int ext_bits) {
    const uint32_t L = 1u << pass.logL;
    uint32_t threads = L / 4 > 128 ? L / 4 : 128;
    if (threads > NTT_THREADS) threads = NTT_THREADS;
    const dim3 grid(1u << (log_n - pass.logL));
    const bool r4 = L >= 4 * threads;  // only when every thread gets a quad
    if (ext_bits < 0) {
        hipLaunchKernelGGL(r4 ? k_ntt_pass<true> : k_ntt_pass<false>, grid,
                           dim3(threads), LDS_BYTES(L), st, pass);
        return;
    }
    NttExtPass ext;
    static_cast<NttPass&>(ext) = pass;
    ext.log_in = log_n - (uint32_t)ext_bits;
    ext.prune = (uint32_t)ext_bits < pass.logL ? (uint32_t)ext_bits : pass.logL;
    hipLaunchKernelGGL((r4 ? k_ntt_pass<true, true> : k_ntt_pass<false, true>),
                       grid, dim3(threads), LDS_BYTES(L), st, ext);
}

// The pass loop of both entry points over 2^log_n elements (1 <= log_n <=
// 28), d_in -> d_out. ext_bits < 0: d_in has 2^log_n elements (and is d_out,
// for the in-place call). ext_bits >= 0: forward only; d_in has
// 2^(log_n - ext_bits) elements, zeros follow.
static int ntt_run(spectre_gpu_ctx* ctx, int dev, const fp256* d_in,
                   fp256* d_out, uint32_t log_n, int ext_bits,
                   const fp256& omega, int inverse, const fp256* coset_gen) {
    DeviceState& ds = ctx->devs[dev];
    const uint32_t n = 1u << log_n;
    NttPlan* plan = nullptr;
    RC_TRY(get_plan(ds, omega, log_n, ctx->ntt_force3, &plan));
    ScratchLayout lay;
    const uint64_t o_tmp = lay.add<fp256>(n);
    const uint64_t o_coset = lay.add<fp256>(coset_gen ? pow_table_elems(n) : 0);
    RC_TRY(ds.d_call.reserve(lay.total));
    fp256* const tmp = (fp256*)(ds.d_call.ptr + o_tmp);
    PowTable ctab{};
    if (coset_gen)  // coset power table (per call; tiny)
        ctab = pow_tables_build(ds, *coset_gen, nullptr, n,
                                (fp256*)(ds.d_call.ptr + o_coset));
    NttPass pass{};
    pass.omega = plan->omega;
    pass.inverse = inverse ? 1 : 0;
    if (inverse) {  // n^{-1}
        fp256 ncanon, nm;
        ff_set_zero(ncanon);
        ncanon.l[log_n >> 5] = 1u << (log_n & 31);
        ff_to_mont<NttFr>(nm, ncanon);
        ff_inv<NttFr>(pass.scale, nm);
    }
    // in -> tmp, tmp in place, tmp -> out; a single pass runs in -> out
    uint32_t done = 0;  // log sizes of the axes already transformed
    for (uint32_t i = 0; i < plan->npass; i++) {
        const bool first = i == 0, last = i == plan->npass - 1;
        pass.in = first ? d_in : tmp;
        pass.out = last ? d_out : tmp;
        pass.twL = plan->tw[i].ptr;
        pass.logL = plan->k[i];
        pass.logS = log_n - done - plan->k[i];
        pass.tw_shift = done;
        pass.last = last;
        if (last) {  // m counts the earlier axes' outputs, the first major
            pass.fin_logB = plan->npass == 3 ? plan->k[1] : 0;
            pass.fin_logA = done - pass.fin_logB;
        }
        const bool coset = coset_gen && (inverse ? last : first);
        pass.coset = coset ? ctab : PowTable{};
        launch_pass(ds.stream, pass, log_n, first ? ext_bits : -1);
        done += plan->k[i];
    }
    return call_finish(ds);
}

int ntt_device(spectre_gpu_ctx* ctx, int dev, fp256* d_data, uint32_t log_n,
               const fp256& omega, int inverse, const fp256* coset_gen) {
    HIP_TRY(hipSetDevice(ctx->devs[dev].device_id));
    if (log_n > 28) {  // BN254 Fr 2-adicity
        set_err("ntt: log_n %u > 28 unsupported (Fr 2-adicity)", log_n);
        return -3;
    }
    if (log_n == 0) return 0;  // DFT of size 1 is the identity; n^{-1} = 1, g^0 = 1
    return ntt_run(ctx, dev, d_data, d_data, log_n, -1, omega, inverse,
                   coset_gen);
}

int ntt_extend_device(spectre_gpu_ctx* ctx, int dev, const fp256* d_coeffs,
                      uint32_t log_n, uint32_t ext_bits, fp256* d_out,
                      const fp256& omega_ext, const fp256* coset_gen) {
    DeviceState& ds = ctx->devs[dev];
    HIP_TRY(hipSetDevice(ds.device_id));
    if (log_n + ext_bits == 0) {  // one element, g^0 = 1: a copy
        if (d_out != d_coeffs)
            HIP_TRY(hipMemcpyAsync(d_out, d_coeffs, sizeof(fp256),
                                   hipMemcpyDeviceToDevice, ds.stream));
        return call_finish(ds);
    }
    return ntt_run(ctx, dev, d_coeffs, d_out, log_n + ext_bits, (int)ext_bits,
                   omega_ext, 0, coset_gen);
}
