// gate.hip — quotient-phase glue over Fr: the gate-expression evaluator and
// the pointwise vector ops, the periodic multiply of divide_by_vanishing_poly
// and the opening phase's linear combination among them.
//
// The kernels compute in GateFr, Fr with the C CIOS multiply, the choice they
// were written and measured under; none has been timed with the asm
// multiply.
#include "internal.hpp"

using GateFr = FrCios;

#define THREADS 256  // vector op

// ---- gate-expression evaluator (quotient phase) -------------
// One launch evaluates a whole custom-gate expression over every row: a
// stack machine whose top-of-stack lives in registers and whose lower slots
// live in LDS (a register-indexed array would spill to scratch — LDS slots
// are strided [slot][tid] so access is conflict-free). The program is tiny
// and wave-uniform; columns are read with rotation (row + rot*rot_scale)
// mod n (n is a power of two).
#define GATE_THREADS 256
__global__ __launch_bounds__(GATE_THREADS) void k_fr_gate_eval(
    const fp256* const* __restrict__ cols, const fp256* __restrict__ consts,
    const uint32_t* __restrict__ prog, uint32_t nops, uint64_t n,
    uint32_t rot_scale, int use_y, fp256 y, fp256* __restrict__ out) {
    extern __shared__ uint4 lds4[];
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const uint32_t T = blockDim.x;
    const uint64_t mask = n - 1;
    fp256 tos;
    ff_set_zero(tos);
    int depth = 0;
    // Same split as lds_split_ld / lds_split_st (ff.hpp), written out: with
    // the high half addressed as low + T the compiler emits other address
    // arithmetic for this kernel, and that has not been measured.
    auto lds_slot_st = [&](int s, const fp256& v) {
        uint4 lo, hi;
        memcpy(&lo, &v.l[0], 16);
        memcpy(&hi, &v.l[4], 16);
        lds4[(2 * s) * T + threadIdx.x] = lo;
        lds4[(2 * s + 1) * T + threadIdx.x] = hi;
    };
    auto lds_slot_ld = [&](int s, fp256& v) {
        uint4 lo = lds4[(2 * s) * T + threadIdx.x];
        uint4 hi = lds4[(2 * s + 1) * T + threadIdx.x];
        memcpy(&v.l[0], &lo, 16);
        memcpy(&v.l[4], &hi, 16);
    };
    for (uint32_t pc = 0; pc < nops; pc++) {
        const uint32_t op = prog[3 * pc];
        const uint32_t a = prog[3 * pc + 1];
        const int32_t b = (int32_t)prog[3 * pc + 2];
        if (op == SPECTRE_GATE_OP_COL || op == SPECTRE_GATE_OP_CONST) {
            if (depth >= 1) lds_slot_st(depth - 1, tos);
            if (op == SPECTRE_GATE_OP_COL) {
                const uint64_t idx =
                    (row + (uint64_t)((int64_t)b * rot_scale + (int64_t)n)) &
                    mask;
                tos = cols[a][idx];
            } else {
                tos = consts[a];
            }
            depth++;
        } else if (op == SPECTRE_GATE_OP_NEG) {
            ff_neg<GateFr>(tos, tos);
        } else {  // binary: (second) op (top)
            fp256 lhs;
            lds_slot_ld(depth - 2, lhs);
            if (op == SPECTRE_GATE_OP_ADD) ff_add<GateFr>(tos, lhs, tos);
            else if (op == SPECTRE_GATE_OP_SUB) ff_sub<GateFr>(tos, lhs, tos);
            else ff_mul<GateFr>(tos, lhs, tos);
            depth--;
        }
    }
    if (use_y) {
        fp256 acc = out[row];
        ff_mul<GateFr>(acc, acc, y);
        ff_add<GateFr>(tos, acc, tos);
    }
    out[row] = tos;
}

int fr_gate_eval_device(spectre_gpu_ctx* ctx, int dev,
                        const fp256* const* cols, uint32_t ncols,
                        const fp256* consts, uint32_t nconst,
                        const uint32_t* program, uint32_t nops, uint64_t n,
                        uint32_t rot_scale, const fp256* y, fp256* d_out) {
    DeviceState& ds = ctx->devs[dev];
    HIP_TRY(hipSetDevice(ds.device_id));
    if (n == 0 || (n & (n - 1)) != 0) {
        set_err("gate_eval: n must be a nonzero power of two");
        return -3;
    }
    // validate the program and compute its maximum stack depth
    int depth = 0, maxd = 0;
    for (uint32_t pc = 0; pc < nops; pc++) {
        const uint32_t op = program[3 * pc];
        const uint32_t a = program[3 * pc + 1];
        const int32_t b = (int32_t)program[3 * pc + 2];
        switch (op) {
            case SPECTRE_GATE_OP_COL:
                if (a >= ncols) { set_err("gate_eval: col %u >= %u", a, ncols); return -3; }
                if ((uint64_t)((int64_t)b * rot_scale < 0
                                   ? -(int64_t)b * rot_scale
                                   : (int64_t)b * rot_scale) >= n) {
                    set_err("gate_eval: rotation %d * %u out of range", b, rot_scale);
                    return -3;
                }
                depth++;
                break;
            case SPECTRE_GATE_OP_CONST:
                if (a >= nconst) { set_err("gate_eval: const %u >= %u", a, nconst); return -3; }
                depth++;
                break;
            case SPECTRE_GATE_OP_NEG:
                if (depth < 1) { set_err("gate_eval: NEG on empty stack"); return -3; }
                break;
            case SPECTRE_GATE_OP_ADD:
            case SPECTRE_GATE_OP_SUB:
            case SPECTRE_GATE_OP_MUL:
                if (depth < 2) { set_err("gate_eval: binary op underflow at pc %u", pc); return -3; }
                depth--;
                break;
            default:
                set_err("gate_eval: bad opcode %u at pc %u", op, pc);
                return -3;
        }
        if (depth > maxd) maxd = depth;
        if (maxd > SPECTRE_GATE_MAX_DEPTH) {
            set_err("gate_eval: stack depth %d > %d", maxd, SPECTRE_GATE_MAX_DEPTH);
            return -3;
        }
    }
    if (depth != 1) {
        set_err("gate_eval: program leaves %d values on the stack (need 1)", depth);
        return -3;
    }
    // device staging: [col ptrs][constants][program]
    ScratchLayout lay;
    const uint64_t o_ptr = lay.add<fp256*>(ncols);
    const uint64_t o_con = lay.add<fp256>(nconst);
    const uint64_t o_prg = lay.add<uint32_t>(3 * (uint64_t)nops);
    RC_TRY(ds.d_call.reserve(lay.total));
    const fp256** const d_cols = (const fp256**)(ds.d_call.ptr + o_ptr);
    fp256* const d_consts = (fp256*)(ds.d_call.ptr + o_con);
    uint32_t* const d_program = (uint32_t*)(ds.d_call.ptr + o_prg);
    HIP_TRY(hipMemcpyAsync(d_cols, cols, ncols * sizeof(fp256*),
                           hipMemcpyHostToDevice, ds.stream));
    if (nconst)
        HIP_TRY(hipMemcpyAsync(d_consts, consts, nconst * sizeof(fp256),
                               hipMemcpyHostToDevice, ds.stream));
    HIP_TRY(hipMemcpyAsync(d_program, program, (size_t)nops * 12,
                           hipMemcpyHostToDevice, ds.stream));
    fp256 yv;
    ff_set_zero(yv);
    if (y) yv = *y;
    const uint32_t lds_bytes =
        (maxd > 1 ? (uint32_t)(maxd - 1) * GATE_THREADS * 32u : 0u);
    hipLaunchKernelGGL(k_fr_gate_eval,
                       dim3((uint32_t)((n + GATE_THREADS - 1) / GATE_THREADS)),
                       dim3(GATE_THREADS), lds_bytes, ds.stream,
                       (const fp256* const*)d_cols, (const fp256*)d_consts,
                       (const uint32_t*)d_program, nops, n,
                       rot_scale, y ? 1 : 0, yv, d_out);
    return call_finish(ds);
}

// ---- pointwise Fr vector ops (quotient-phase gate-eval glue) --------------
__global__ void k_fr_vec_op(int op, const fp256* __restrict__ a,
                            const fp256* __restrict__ b, fp256 c,
                            fp256* __restrict__ out, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fp256 r, va = a[i];
    switch (op) {
        case SPECTRE_VEC_ADD: ff_add<GateFr>(r, va, b[i]); break;
        case SPECTRE_VEC_SUB: ff_sub<GateFr>(r, va, b[i]); break;
        case SPECTRE_VEC_MUL: ff_mul<GateFr>(r, va, b[i]); break;
        case SPECTRE_VEC_SCALE: ff_mul<GateFr>(r, va, c); break;
        default: {  // ADD_SCALED
            fp256 t;
            ff_mul<GateFr>(t, b[i], c);
            ff_add<GateFr>(r, va, t);
        }
    }
    out[i] = r;
}

int fr_vec_op_device(spectre_gpu_ctx* ctx, int dev, int op, const fp256* d_a,
                     const fp256* d_b, const fp256* c, fp256* d_out,
                     uint64_t n) {
    DeviceState& ds = ctx->devs[dev];
    HIP_TRY(hipSetDevice(ds.device_id));
    if (n == 0) return 0;
    fp256 cv;
    ff_set_zero(cv);
    if (c) cv = *c;
    hipLaunchKernelGGL(k_fr_vec_op,
                       dim3((uint32_t)((n + THREADS - 1) / THREADS)),
                       dim3(THREADS), 0, ds.stream, op, d_a, d_b, cv, d_out,
                       n);
    return call_finish(ds);
}

// ---- out[i] = sum_k c[k] * p[k][i] (multiopen's sums in y and v) -----------
// The pointers and coefficients travel in the kernel arguments (32 * 8 +
// 32 * 32 = 1280 B), so nothing is staged. Row i runs in lane i, two 16-byte
// loads per element; the column loop is wave-uniform to the run-time m and
// the accumulator stays in registers: no LDS, no scratch. The kernel
// streams, so what matters is the loads in flight per lane: the loop takes
// LINCOMB_AHEAD polynomials per trip and issues all their loads before the
// first multiply (1 = a round trip to memory per polynomial). Measured, 1, 2
// and 4 are within 1 % of each other at m = 8 and 32 (eight waves per SIMD
// already keep the memory system busy); 2 is kept for m = 2, where it is up
// to 5 % ahead, at 54 VGPRs; 8 spills (DESIGN.md "Multiopen"). out may equal
// any input (hence no __restrict__): a lane reads row i of every input
// before it writes row i, and touches no other row.
#ifndef LINCOMB_AHEAD
#define LINCOMB_AHEAD 2
#endif
struct LincombArgs {
    const fp256* p[SPECTRE_OPEN_MAX_POLYS];
    fp256 c[SPECTRE_OPEN_MAX_POLYS];
};
__global__ __launch_bounds__(THREADS) void k_fr_lincomb(
    LincombArgs a, uint32_t m, fp256* out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fp256 acc;
    ff_set_zero(acc);
#pragma unroll 1
    for (uint32_t k0 = 0; k0 < m; k0 += LINCOMB_AHEAD) {
        fp256 v[LINCOMB_AHEAD];
#pragma unroll
        for (uint32_t j = 0; j < LINCOMB_AHEAD; j++)
            if (k0 + j < m) v[j] = a.p[k0 + j][i];
#pragma unroll
        for (uint32_t j = 0; j < LINCOMB_AHEAD; j++) {
            if (k0 + j < m) {
                fp256 t;
                ff_mul<GateFr>(t, v[j], a.c[k0 + j]);
                ff_add<GateFr>(acc, acc, t);
            }
        }
    }
    out[i] = acc;
}

int fr_lincomb_device(spectre_gpu_ctx* ctx, int dev,
                      const fp256* const* d_polys, const fp256* coeffs,
                      uint32_t m, fp256* d_out, uint64_t n) {
    DeviceState& ds = ctx->devs[dev];
    HIP_TRY(hipSetDevice(ds.device_id));
    if (n == 0) return 0;
    LincombArgs a;
    for (uint32_t k = 0; k < SPECTRE_OPEN_MAX_POLYS; k++) {
        a.p[k] = k < m ? d_polys[k] : nullptr;
        if (k < m) a.c[k] = coeffs[k];
        else ff_set_zero(a.c[k]);
    }
    hipLaunchKernelGGL(k_fr_lincomb,
                       dim3((uint32_t)((n + THREADS - 1) / THREADS)),
                       dim3(THREADS), 0, ds.stream, a, m, d_out, n);
    return call_finish(ds);
}

// ---- out[i] = a[i] * table[i mod period] (divide_by_vanishing_poly) -------
// The table (at most 2 KiB) travels in the kernel arguments, filled to its
// full length by repetition so the index needs only one mask. out may alias
// a (hence no __restrict__): every thread reads its element before it writes.
struct FrPeriodTable {
    fp256 t[SPECTRE_VEC_PERIOD_MAX];
};
__global__ void k_fr_vec_mul_periodic(const fp256* a, FrPeriodTable table,
                                      fp256* out, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fp256 r;
    ff_mul<GateFr>(r, a[i], table.t[i & (SPECTRE_VEC_PERIOD_MAX - 1)]);
    out[i] = r;
}

int fr_vec_mul_periodic_device(spectre_gpu_ctx* ctx, int dev,
                               const fp256* d_a, const fp256* table,
                               uint32_t period, fp256* d_out, uint64_t n) {
    DeviceState& ds = ctx->devs[dev];
    HIP_TRY(hipSetDevice(ds.device_id));
    if (n == 0) return 0;
    FrPeriodTable tab;
    for (uint32_t j = 0; j < SPECTRE_VEC_PERIOD_MAX; j++)
        tab.t[j] = table[j & (period - 1)];
    hipLaunchKernelGGL(k_fr_vec_mul_periodic,
                       dim3((uint32_t)((n + THREADS - 1) / THREADS)),
                       dim3(THREADS), 0, ds.stream, d_a, tab, d_out, n);
    return call_finish(ds);
}
