// perm.hip — the permutation argument's per-row terms and the row-power
// column they need (halo2 plonk/permutation/prover.rs and evaluation.rs):
//   fr_powers            out[i] = c * g^i
//   fr_permutation_terms den[i] = prod_j (v_j[i] + beta*sigma_j[i]        + gamma)
//                        num[i] = prod_j (v_j[i] + beta*delta0*delta^j*omega^i + gamma)
// The terms feed fr_grand_product (poly.hip); the powers column of
// (zeta, omega_ext) is the X of the extended-domain permutation constraint, an
// ordinary gate_eval column.
//
// Row powers come from the two-level table ntt.hip uses for its twiddles,
//   g^i = T1[i & 0xfff] * T2[i >> 12],
// built per call on the stream (4096 + ceil(n / 4096) entries, 0.4% of the
// rows at 2^20, in one launch) for ANY field element g: an NTT plan's cached
// tables exist only for roots of unity and only for exponents below that
// plan's n, so they are not looked at here. fr_powers
// folds c into T2 and spends one multiply per row; the terms kernel spends
// one multiply on omega^i and shares it among the m columns.
//
// Both kernels put row i in lane i: every column access is the two 16-byte
// loads per element of k_fr_gate_eval, no LDS, no scratch. They compute in
// PermFr, Fr with the C CIOS multiply, as gate.hip does; the asm multiply has
// not been timed here.
#include "internal.hpp"

using PermFr = FrCios;

#define THREADS 256
#define PW_LOW_BITS 12
#define PW_LOW (1u << PW_LOW_BITS)
#define PW_LOW_MASK (PW_LOW - 1u)

// ---- the two power tables, one launch ---------------------------------------
// A table entry g^e is a product of one constant per base-4 digit of e,
// c[w][d - 1] = g^(d * 4^w): the host squares its way up the 14 windows (a
// few dozen multiplies) and hands them over in the kernel arguments, so an
// entry costs at most 6 (T1) or 8 (T2) dependent multiplies where a
// square-and-multiply chain per entry costs up to 24 — the build is a
// latency chain on a handful of waves, and its depth is its time. T1's
// exponent j uses windows 0..5, T2's exponent 4096 j windows 6..13.
#define PW_WINDOWS 14
#define PW_LOW_WINDOWS (PW_LOW_BITS / 2)
struct PowWindows {
    fp256 c[PW_WINDOWS][3];
};

// Blocks [0, nb1): t1[j] = g^j, j < t1n. Blocks from nb1: t2[j] = scale *
// g^(4096 j), j < t2n. nwin1 / nwin2 = base-4 digits of t1n - 1 / t2n - 1.
__global__ __launch_bounds__(THREADS) void k_perm_pow_tables(
    PowWindows pw, fp256 scale, fp256* __restrict__ t1, uint32_t t1n,
    uint32_t nwin1, fp256* __restrict__ t2, uint32_t t2n, uint32_t nwin2,
    uint32_t nb1) {
    const bool high = blockIdx.x >= nb1;
    const uint32_t j =
        (blockIdx.x - (high ? nb1 : 0u)) * blockDim.x + threadIdx.x;
    if (j >= (high ? t2n : t1n)) return;
    const uint32_t w0 = high ? PW_LOW_WINDOWS : 0u;
    const uint32_t nwin = high ? nwin2 : nwin1;
    fp256 acc;
    if (high) acc = scale;
    else ff_set_one<PermFr>(acc);
#pragma unroll 1
    for (uint32_t w = 0; w < nwin; w++) {
        const uint32_t d = (j >> (2 * w)) & 3u;
        fp256 f, t;
#pragma unroll
        for (int i = 0; i < 8; i++)
            f.l[i] = d == 1 ? pw.c[w0 + w][0].l[i]
                            : (d == 2 ? pw.c[w0 + w][1].l[i]
                                      : pw.c[w0 + w][2].l[i]);
        ff_mul<PermFr>(t, acc, f);
#pragma unroll
        for (int i = 0; i < 8; i++) acc.l[i] = d ? t.l[i] : acc.l[i];
    }
    (high ? t2 : t1)[j] = acc;
}

static uint32_t base4_digits(uint32_t x) {
    uint32_t d = 0;
    for (; x; x >>= 2) d++;
    return d;
}

// T1 (min(n, 4096) entries, g^j) || T2 (ceil(n / 4096) entries,
// scale * g^(4096 j)) into ds.d_perm_pow; enqueued, not synchronized.
static int build_power_tables(DeviceState& ds, const fp256& g,
                              const fp256& scale, uint64_t n,
                              const fp256** T1, const fp256** T2) {
    const uint32_t t1n = n < PW_LOW ? (uint32_t)n : PW_LOW;
    const uint32_t t2n = (uint32_t)((n + PW_LOW - 1) >> PW_LOW_BITS);
    RC_TRY(ds.d_perm_pow.reserve((size_t)PW_LOW + t2n));
    PowWindows pw;
    fp256 b = g;
    for (int w = 0; w < PW_WINDOWS; w++) {
        pw.c[w][0] = b;
        ff_sqr<PermFr>(pw.c[w][1], b);
        ff_mul<PermFr>(pw.c[w][2], pw.c[w][1], b);
        ff_sqr<PermFr>(b, pw.c[w][1]);
    }
    fp256* const t1 = ds.d_perm_pow.ptr;
    fp256* const t2 = t1 + PW_LOW;
    const uint32_t nb1 = (t1n + THREADS - 1) / THREADS;
    const uint32_t nb2 = (t2n + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(k_perm_pow_tables, dim3(nb1 + nb2), dim3(THREADS), 0,
                       ds.stream, pw, scale, t1, t1n, base4_digits(t1n - 1),
                       t2, t2n, base4_digits(t2n - 1), nb1);
    *T1 = t1;
    *T2 = t2;
    return 0;
}

// ---- out[i] = c * g^i ------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_fr_powers(
    const fp256* __restrict__ T1, const fp256* __restrict__ T2,
    fp256* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fp256 r;
    ff_mul<PermFr>(r, T1[(uint32_t)i & PW_LOW_MASK], T2[i >> PW_LOW_BITS]);
    out[i] = r;
}

int fr_powers_device(spectre_gpu_ctx* ctx, int dev, const fp256& c,
                     const fp256& g, fp256* d_out, uint64_t n) {
    DeviceState& ds = ctx->devs[dev];
    HIP_TRY(hipSetDevice(ds.device_id));
    if (n == 0) return 0;
    const fp256 *T1, *T2;
    RC_TRY(build_power_tables(ds, g, c, n, &T1, &T2));
    hipLaunchKernelGGL(k_fr_powers,
                       dim3((uint32_t)((n + THREADS - 1) / THREADS)),
                       dim3(THREADS), 0, ds.stream, T1, T2, d_out, n);
    HIP_TRY(hipStreamSynchronize(ds.stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- permutation terms -----------------------------------------------------
// The column pointers and every constant travel in the kernel arguments
// (16 pointers + 10 elements = 448 B), so no staging copy precedes the launch.
struct PermArgs {
    const fp256* v[SPECTRE_PERM_MAX_COLS];
    const fp256* s[SPECTRE_PERM_MAX_COLS];
    fp256 bd[SPECTRE_PERM_MAX_COLS];  // beta * delta0 * delta^j
    fp256 beta, gamma;
};

// One factor pair of column j: fd = v + beta*sigma + gamma, fn = v + bd*w + gamma.
__device__ __forceinline__ void perm_factors(const PermArgs& a, uint32_t j,
                                             uint64_t i, const fp256& w,
                                             fp256& fn, fp256& fd) {
    fp256 vg = a.v[j][i], t;
    ff_add<PermFr>(vg, vg, a.gamma);
    ff_mul<PermFr>(t, a.s[j][i], a.beta);
    ff_add<PermFr>(fd, vg, t);
    ff_mul<PermFr>(t, w, a.bd[j]);
    ff_add<PermFr>(fn, vg, t);
}

// The column loop is wave-uniform (m and the per-column arguments are
// scalars), so both running products stay in registers; asking for it
// unrolled per m changes neither the register count nor the scratch (none).
__global__ __launch_bounds__(THREADS) void k_fr_perm_terms(
    PermArgs a, uint32_t m, const fp256* __restrict__ T1,
    const fp256* __restrict__ T2, fp256* __restrict__ num,
    fp256* __restrict__ den, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fp256 w;  // omega^i
    ff_mul<PermFr>(w, T1[(uint32_t)i & PW_LOW_MASK], T2[i >> PW_LOW_BITS]);
    fp256 pn, pd;
    perm_factors(a, 0, i, w, pn, pd);
#pragma unroll 1
    for (uint32_t j = 1; j < m; j++) {
        fp256 fn, fd;
        perm_factors(a, j, i, w, fn, fd);
        ff_mul<PermFr>(pn, pn, fn);
        ff_mul<PermFr>(pd, pd, fd);
    }
    num[i] = pn;
    den[i] = pd;
}

int fr_permutation_terms_device(spectre_gpu_ctx* ctx, int dev,
                                const fp256* const* d_values,
                                const fp256* const* d_sigmas, uint32_t m,
                                const fp256& beta, const fp256& gamma,
                                const fp256& omega, const fp256& delta0,
                                const fp256& delta, fp256* d_num, fp256* d_den,
                                uint64_t n) {
    DeviceState& ds = ctx->devs[dev];
    HIP_TRY(hipSetDevice(ds.device_id));
    if (n == 0) return 0;
    PermArgs a;
    a.beta = beta;
    a.gamma = gamma;
    fp256 bd;
    ff_mul<PermFr>(bd, beta, delta0);
    for (uint32_t j = 0; j < SPECTRE_PERM_MAX_COLS; j++) {
        a.v[j] = j < m ? d_values[j] : nullptr;
        a.s[j] = j < m ? d_sigmas[j] : nullptr;
        a.bd[j] = bd;
        ff_mul<PermFr>(bd, bd, delta);
    }
    fp256 one;
    ff_set_one<PermFr>(one);
    const fp256 *T1, *T2;
    RC_TRY(build_power_tables(ds, omega, one, n, &T1, &T2));
    hipLaunchKernelGGL(k_fr_perm_terms,
                       dim3((uint32_t)((n + THREADS - 1) / THREADS)),
                       dim3(THREADS), 0, ds.stream, a, m, T1, T2, d_num, d_den,
                       n);
    HIP_TRY(hipStreamSynchronize(ds.stream));
    HIP_TRY(hipGetLastError());
    return 0;
}
