// perm.hip — the permutation argument's per-row terms and the row-power
// column they need (halo2 plonk/permutation/prover.rs and evaluation.rs):
//   fr_powers            out[i] = c * g^i
//   fr_permutation_terms den[i] = prod_j (v_j[i] + beta*sigma_j[i]        + gamma)
//                        num[i] = prod_j (v_j[i] + beta*delta0*delta^j*omega^i + gamma)
// The terms feed fr_grand_product (poly.hip); the powers column of
// (zeta, omega_ext) is the X of the extended-domain permutation constraint, an
// ordinary gate_eval column.
//
// Row powers g^i come from the two-level table of powtab.hpp, built per call
// on the stream (4096 + ceil(n / 4096) entries, 0.4% of the rows at 2^20, in
// one launch) for ANY field element g: an NTT plan's cached table exists only
// for roots of unity and only for exponents below that plan's n, so it is not
// looked at here. fr_powers folds c into T2: one multiply per row; the terms
// kernel spends one multiply on omega^i and shares it among the m columns.
//
// Both kernels put row i in lane i: every column access is the two 16-byte
// loads per element of k_fr_gate_eval, no LDS, no scratch. They compute in
// PermFr, Fr with the C CIOS multiply, as gate.hip does; the asm multiply has
// not been timed here.
#include "internal.hpp"

using PermFr = FrCios;

#define THREADS 256

// ---- out[i] = c * g^i ------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_fr_powers(
    PowTable tab, fp256* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fp256 r;
    pow_lookup<PermFr>(r, tab, i);
    out[i] = r;
}

int fr_powers_device(spectre_gpu_ctx* ctx, int dev, const fp256& c,
                     const fp256& g, fp256* d_out, uint64_t n) {
    DeviceState& ds = ctx->devs[dev];
    HIP_TRY(hipSetDevice(ds.device_id));
    if (n == 0) return 0;
    RC_TRY(ds.d_call.reserve(pow_table_elems(n) * sizeof(fp256)));
    const PowTable tab = pow_tables_build(ds, g, &c, n, (fp256*)ds.d_call.ptr);
    hipLaunchKernelGGL(k_fr_powers,
                       dim3((uint32_t)((n + THREADS - 1) / THREADS)),
                       dim3(THREADS), 0, ds.stream, tab, d_out, n);
    return call_finish(ds);
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
    PermArgs a, uint32_t m, PowTable tab, fp256* __restrict__ num,
    fp256* __restrict__ den, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fp256 w;  // omega^i
    pow_lookup<PermFr>(w, tab, i);
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
    RC_TRY(ds.d_call.reserve(pow_table_elems(n) * sizeof(fp256)));
    const PowTable tab =
        pow_tables_build(ds, omega, nullptr, n, (fp256*)ds.d_call.ptr);
    hipLaunchKernelGGL(k_fr_perm_terms,
                       dim3((uint32_t)((n + THREADS - 1) / THREADS)),
                       dim3(THREADS), 0, ds.stream, a, m, tab, d_num, d_den, n);
    return call_finish(ds);
}
