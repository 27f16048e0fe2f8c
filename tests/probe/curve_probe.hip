// curve_probe.hip — TEST INFRASTRUCTURE, not part of the product ABI.
//
// Calls ff_dot2 and the XYZZ point forms of g1.hpp one at a time, so the suite
// can compare each with Python bigints at chosen operands
// (tests/test_dot2_edges.py, tests/test_xyzz_curve.py). Built by
// spectre_amd/csrc/Makefile into spectre_amd/libspectre_curveprobe.so with the
// product's flags, beside field_probe.hip, which it leaves as it is.
//
// Two entry points of one signature, the same code behind both:
//   curveprobe_device: one thread per element, 256-thread blocks; returns the
//                      first failing HIP error code, 0 on success
//   curveprobe_host:   a plain loop through the host build of the headers;
//                      makes no HIP call
// Both return -1, before touching anything, for a request they do not serve.
// Element sizes in bytes (field: 0 Fq, 1 Fr, 2 FrCios; curve ops Fq only):
//   DOT2       a 64 (a | b),  b 64 (c | d),   out 32: a*b + c*d
//   DOT2CHAIN  the same; x0 = a, then 32 steps x = dot2(x, b, c, d) (even) or
//              x = dot2(a, x, x, d) (odd), the output over an operand
//   X_DBL      a 128 (XYZZ),  b unused,       out 128
//   X_MADD     a 128,         b 64 (affine),  out 128
//   X_ADD      a 128,         b 128,          out 128
//   X_TO_JAC   a 128,         b unused,       out 96 (Jacobian)
// A curve op mutates a copy of a[i] and stores that to out[i]. No global
// state; loading the library makes no HIP call.
#include <type_traits>

#include "g1.hpp"

enum { OP_DOT2 = 0, OP_DOT2CHAIN, OP_FIELD_END,
       OP_X_DBL = 16, OP_X_MADD, OP_X_ADD, OP_X_TO_JAC, OP_X_END };
enum { F_FQ = 0, F_FR, F_FRCIOS, F_END };
#define CHAIN_STEPS 32
#define PROBE_THREADS 256
#define PROBE_MAX_N (1ull << 24)

constexpr bool op_is_curve(int op) { return op >= OP_X_DBL && op < OP_X_END; }

struct fp_pair {
    fp256 u, v;
};

template <class C, int OP>
FF_HD void probe_elem(const void* a, const void* b, void* out, uint64_t i) {
    if constexpr (OP == OP_DOT2 || OP == OP_DOT2CHAIN) {
        const fp_pair ab = ((const fp_pair*)a)[i], cd = ((const fp_pair*)b)[i];
        fp256 x;
        if constexpr (OP == OP_DOT2) {
            ff_dot2<C>(x, ab.u, ab.v, cd.u, cd.v);
        } else {
            x = ab.u;
            for (int s = 0; s < CHAIN_STEPS; s += 2) {
                ff_dot2<C>(x, x, ab.v, cd.u, cd.v);
                ff_dot2<C>(x, ab.u, x, x, cd.v);
            }
        }
        ((fp256*)out)[i] = x;
    } else if constexpr (OP == OP_X_TO_JAC) {
        g1_jac j;
        g1x_to_jac(j, ((const g1_xyzz*)a)[i]);
        ((g1_jac*)out)[i] = j;
    } else {
        g1_xyzz p = ((const g1_xyzz*)a)[i];
        if constexpr (OP == OP_X_DBL) g1x_dbl_ip(p);
        else if constexpr (OP == OP_X_MADD) g1x_madd_ip(p, ((const g1_affine*)b)[i]);
        else {
            static_assert(OP == OP_X_ADD, "unknown op");
            g1x_add_ip(p, ((const g1_xyzz*)b)[i]);
        }
        ((g1_xyzz*)out)[i] = p;
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

// f(C{}, std::integral_constant<int, OP>{}) for a served (op, field)
template <class C, class F> static void with_op(int op, F f) {
    switch (op) {
#define PROBE_OP(O)                                                  \
    case O:                                                          \
        if constexpr (!op_is_curve(O) || std::is_same<C, Fq>::value) \
            f(C{}, std::integral_constant<int, O>{});                \
        return;
        PROBE_OP(OP_DOT2) PROBE_OP(OP_DOT2CHAIN) PROBE_OP(OP_X_DBL)
        PROBE_OP(OP_X_MADD) PROBE_OP(OP_X_ADD) PROBE_OP(OP_X_TO_JAC)
#undef PROBE_OP
    }
}
template <class F> static void with_field_op(int op, int field, F f) {
    switch (field) {
        case F_FQ: return with_op<Fq>(op, f);
        case F_FR: return with_op<Fr>(op, f);
        case F_FRCIOS: return with_op<FrCios>(op, f);
    }
}

// element sizes of a served request; false for any other
static bool request_shape(int op, int field, size_t& sa, size_t& sb,
                          size_t& so) {
    if (field < 0 || field >= F_END) return false;
    if (op_is_curve(op)) {
        if (field != F_FQ) return false;
        sa = sizeof(g1_xyzz);
        sb = op == OP_X_MADD ? sizeof(g1_affine)
           : op == OP_X_ADD ? sizeof(g1_xyzz) : 0;
        so = op == OP_X_TO_JAC ? sizeof(g1_jac) : sizeof(g1_xyzz);
        return true;
    }
    if (op < 0 || op >= OP_FIELD_END) return false;
    sa = sb = sizeof(fp_pair);
    so = sizeof(fp256);
    return true;
}

extern "C" int curveprobe_device(int op, int field, const void* a,
                                 const void* b, void* out, uint64_t n) {
    size_t sa, sb, so;
    if (!request_shape(op, field, sa, sb, so)) return -1;
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

extern "C" int curveprobe_host(int op, int field, const void* a, const void* b,
                               void* out, uint64_t n) {
    size_t sa, sb, so;
    if (!request_shape(op, field, sa, sb, so)) return -1;
    if (!a || !out || (sb && !b) || n > PROBE_MAX_N) return -1;
    with_field_op(op, field, [&](auto c, auto o) {
        for (uint64_t i = 0; i < n; i++)
            probe_elem<decltype(c), decltype(o)::value>(a, b, out, i);
    });
    return 0;
}
