// field_probe.hip — TEST INFRASTRUCTURE, not part of the product ABI.
//
// Calls the primitives of ff.hpp and g1.hpp one at a time, so the suite can
// compare each with Python bigints at chosen operands
// (tests/test_field_probe.py). Built by spectre_amd/csrc/Makefile into
// spectre_amd/libspectre_ffprobe.so with the product's flags, so the asm
// multiply is compiled as it is in libspectre_gpu.so.
//
// Two entry points of one signature:
//   ffprobe_device: one thread per element, 256-thread blocks; returns the
//                   first failing HIP error code, 0 on success
//   ffprobe_host:   the same op in a plain loop through the host build of the
//                   headers; makes no HIP call
// Both return -1, before touching anything, for a request they do not serve.
// Element sizes in bytes:
//   field ops  a 32, b 32 (read by two-operand ops only), out 32
//   G1_DBL     a 96 (Jacobian), b unused,         out 96
//   G1_MADD    a 96,            b 64 (affine),    out 96
//   G1_ADD     a 96,            b 96,             out 96
// A curve op mutates a copy of a[i], its accumulator, and stores that to
// out[i]. No global state; loading the library makes no HIP call.
#include <type_traits>

#include "g1.hpp"

enum {
    OP_MUL = 0, OP_SQR, OP_ADD, OP_SUB, OP_NEG, OP_INV, OP_TO_MONT,
    OP_FROM_MONT, OP_POW_U32,  // exponent = low limb of b
    OP_MUL_CIOS,               // device only, Fq and Fr: ff_mul_cios by name
    OP_MULCHAIN,               // x0 = a, x_{i+1} = x_i * (i odd ? a : b), 32 steps
    OP_SQRCHAIN,               // x0 = a, x_{i+1} = x_i^2, 32 steps
    OP_FIELD_END,
    OP_G1_DBL = 16, OP_G1_MADD, OP_G1_ADD, OP_G1_END
};
enum { F_FQ = 0, F_FR, F_FRCIOS, F_END };
#define CHAIN_STEPS 32
#define PROBE_THREADS 256
#define PROBE_MAX_N (1ull << 24)

constexpr bool op_is_curve(int op) { return op >= OP_G1_DBL && op < OP_G1_END; }
constexpr bool op_reads_b(int op) {
    return op == OP_MUL || op == OP_ADD || op == OP_SUB || op == OP_POW_U32 ||
           op == OP_MUL_CIOS || op == OP_MULCHAIN || op == OP_G1_MADD ||
           op == OP_G1_ADD;
}

// ---- the ops, host and device ----------------------------------------------
template <class C, int OP>
FF_HD void field_op(fp256& o, const fp256& a, const fp256& b) {
    if constexpr (OP == OP_MUL) ff_mul<C>(o, a, b);
    else if constexpr (OP == OP_SQR) ff_sqr<C>(o, a);
    else if constexpr (OP == OP_ADD) ff_add<C>(o, a, b);
    else if constexpr (OP == OP_SUB) ff_sub<C>(o, a, b);
    else if constexpr (OP == OP_NEG) ff_neg<C>(o, a);
    else if constexpr (OP == OP_INV) ff_inv<C>(o, a);
    else if constexpr (OP == OP_TO_MONT) ff_to_mont<C>(o, a);
    else if constexpr (OP == OP_FROM_MONT) ff_from_mont<C>(o, a);
    else if constexpr (OP == OP_POW_U32) ff_pow_u32<C>(o, a, b.l[0]);
    else if constexpr (OP == OP_MUL_CIOS) ff_mul_cios<C>(o, a, b);
    else if constexpr (OP == OP_MULCHAIN) {
        // unrolled, so on the device the asm blocks of one multiply are
        // followed at once by those of the next
        fp256 x = a;
#pragma unroll
        for (int i = 0; i < CHAIN_STEPS; i++) ff_mul<C>(x, x, (i & 1) ? a : b);
        o = x;
    } else {
        static_assert(OP == OP_SQRCHAIN, "unknown field op");
        fp256 x = a;
#pragma unroll
        for (int i = 0; i < CHAIN_STEPS; i++) ff_sqr<C>(x, x);
        o = x;
    }
}
template <int OP>
FF_HD void curve_op(g1_jac& p, const void* b, uint64_t i) {
    if constexpr (OP == OP_G1_DBL) g1j_dbl_ip(p);
    else if constexpr (OP == OP_G1_MADD) g1j_madd_ip(p, ((const g1_affine*)b)[i]);
    else {
        static_assert(OP == OP_G1_ADD, "unknown curve op");
        g1j_add_ip(p, ((const g1_jac*)b)[i]);
    }
}
// element i of an op, field or curve; C is ignored by the curve ops (Fq)
template <class C, int OP>
FF_HD void probe_elem(const void* a, const void* b, void* out, uint64_t i) {
    if constexpr (op_is_curve(OP)) {
        g1_jac p = ((const g1_jac*)a)[i];
        curve_op<OP>(p, b, i);
        ((g1_jac*)out)[i] = p;
    } else {
        fp256 va = ((const fp256*)a)[i], vb, r;
        if constexpr (op_reads_b(OP)) vb = ((const fp256*)b)[i];
        else ff_set_zero(vb);
        field_op<C, OP>(r, va, vb);
        ((fp256*)out)[i] = r;
    }
}

template <class C, int OP>
__global__ __launch_bounds__(PROBE_THREADS) void k_probe(
    const void* __restrict__ a, const void* __restrict__ b,
    void* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    probe_elem<C, OP>(a, b, out, i);
}

// ---- run-time (op, field) -> compile-time <C, OP> ---------------------------
// f(C{}, std::integral_constant<int, OP>{}) for a known op and field, else
// false; the curve ops exist over Fq only
template <class C, class F> static bool with_op(int op, F f) {
    switch (op) {
#define PROBE_OP(O)                                                  \
    case O:                                                          \
        if constexpr (!op_is_curve(O) || std::is_same<C, Fq>::value) \
            f(C{}, std::integral_constant<int, O>{});                \
        return true;
        PROBE_OP(OP_MUL) PROBE_OP(OP_SQR) PROBE_OP(OP_ADD) PROBE_OP(OP_SUB)
        PROBE_OP(OP_NEG) PROBE_OP(OP_INV) PROBE_OP(OP_TO_MONT)
        PROBE_OP(OP_FROM_MONT) PROBE_OP(OP_POW_U32) PROBE_OP(OP_MUL_CIOS)
        PROBE_OP(OP_MULCHAIN) PROBE_OP(OP_SQRCHAIN) PROBE_OP(OP_G1_DBL)
        PROBE_OP(OP_G1_MADD) PROBE_OP(OP_G1_ADD)
#undef PROBE_OP
    }
    return false;
}
template <class F> static bool with_field_op(int op, int field, F f) {
    switch (field) {
        case F_FQ: return with_op<Fq>(op, f);
        case F_FR: return with_op<Fr>(op, f);
        case F_FRCIOS: return with_op<FrCios>(op, f);
    }
    return false;
}

// element sizes of a served request; false for any other
static bool request_shape(int op, int field, bool device, size_t& sa,
                          size_t& sb, size_t& so) {
    if (field < 0 || field >= F_END) return false;
    if (op_is_curve(op)) {
        if (field != F_FQ) return false;
        sa = so = sizeof(g1_jac);
        sb = op == OP_G1_MADD ? sizeof(g1_affine)
           : op == OP_G1_ADD ? sizeof(g1_jac) : 0;
        return true;
    }
    if (op < 0 || op >= OP_FIELD_END) return false;
    // the CIOS by name: where ff_mul is something else, the device's Fq and Fr
    if (op == OP_MUL_CIOS && (!device || field == F_FRCIOS)) return false;
    sa = so = sizeof(fp256);
    sb = op_reads_b(op) ? sizeof(fp256) : 0;
    return true;
}

extern "C" int ffprobe_device(int op, int field, const void* a, const void* b,
                              void* out, uint64_t n) {
    size_t sa, sb, so;
    if (!request_shape(op, field, true, sa, sb, so)) return -1;
    if (!a || !out || (sb && !b) || n > PROBE_MAX_N) return -1;
    if (n == 0) return 0;
    void *d_a = nullptr, *d_b = nullptr, *d_out = nullptr;
    int rc = 0;
    // first failure wins and skips what follows; the frees run either way
#define PROBE_TRY(call)                                   \
    do {                                                  \
        if (rc == 0) {                                    \
            hipError_t e_ = (call);                       \
            if (e_ != hipSuccess) rc = (int)e_;           \
        }                                                 \
    } while (0)
    PROBE_TRY(hipMalloc(&d_a, sa * n));
    if (sb) PROBE_TRY(hipMalloc(&d_b, sb * n));
    PROBE_TRY(hipMalloc(&d_out, so * n));
    PROBE_TRY(hipMemcpy(d_a, a, sa * n, hipMemcpyHostToDevice));
    if (sb) PROBE_TRY(hipMemcpy(d_b, b, sb * n, hipMemcpyHostToDevice));
    PROBE_TRY(hipMemset(d_out, 0xa5, so * n));
    if (rc == 0) {
        const dim3 grid((uint32_t)((n + PROBE_THREADS - 1) / PROBE_THREADS));
        with_field_op(op, field, [&](auto c, auto o) {
            hipLaunchKernelGGL((k_probe<decltype(c), decltype(o)::value>),
                               grid, dim3(PROBE_THREADS), 0, 0,
                               (const void*)d_a, (const void*)d_b, d_out, n);
        });
    }
    PROBE_TRY(hipGetLastError());
    PROBE_TRY(hipDeviceSynchronize());
    PROBE_TRY(hipMemcpy(out, d_out, so * n, hipMemcpyDeviceToHost));
#undef PROBE_TRY
    void* const bufs[3] = {d_a, d_b, d_out};
    for (int i = 0; i < 3; i++) {
        if (!bufs[i]) continue;
        hipError_t e = hipFree(bufs[i]);
        if (rc == 0 && e != hipSuccess) rc = (int)e;
    }
    return rc;
}

extern "C" int ffprobe_host(int op, int field, const void* a, const void* b,
                            void* out, uint64_t n) {
    size_t sa, sb, so;
    if (!request_shape(op, field, false, sa, sb, so)) return -1;
    if (!a || !out || (sb && !b) || n > PROBE_MAX_N) return -1;
    with_field_op(op, field, [&](auto c, auto o) {
        for (uint64_t i = 0; i < n; i++)
            probe_elem<decltype(c), decltype(o)::value>(a, b, out, i);
    });
    return 0;
}
