// ff.hpp — BN254 prime-field arithmetic, 8x32-bit limbs, Montgomery form.
//
// PRODUCT CODE (part of libspectre_gpu.so). Compiles both as HIP device code
// (gfx950) and as plain host C++ (the FFI's final-reduction path). 32-bit
// limbs are chosen for the CDNA4 VALU: a 256-bit Montgomery multiply (CIOS)
// lowers to chains of 32x32->64 multiply-adds (v_mad_u64_u32 class), which is
// the native integer-multiply shape on gfx950. This is deliberately a
// DIFFERENT limb decomposition from the CPU oracle's 4x64/__int128 so the two
// implementations cannot share a limb-level bug.
//
// Memory format (= halo2curves-axiom 0.5.2 memory image, the reference's
// arithmetic dependency — /root/reference/Cargo.toml:53): a field element is
// 32 little-endian bytes of the Montgomery residue a*2^256 mod m, i.e. the
// limb array IS the byte image on a little-endian machine (both host and
// gfx950 are LE). "Canonical" = 32 LE bytes of a itself (Fr::to_repr()).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#include <hip/hip_runtime.h>
#define FF_HD __host__ __device__ __forceinline__
#else
#define FF_HD inline
#endif

struct fp256 {
    uint32_t l[8];
};

// ---- constant providers -----------------------------------------------------
// Constants derived from the published alt_bn128 moduli (values verified
// against tests/golden fixtures; see tests/golden/bn254_ref.py).
// kAsmMul: which multiply ff_mul<C> is in device code, the asm column form
// (true) or the compiled CIOS (false). The host always runs the CIOS.
// kChainAddSub: which form ff_add / ff_sub / ff_cond_sub_mod take, host and
// device: branch-free 32-bit carry chains with the correction selected by a
// mask (true), or 64-bit limb arithmetic with the correction behind a branch
// (false). Same bytes either way; the choice is per field because it moves
// register allocation in opposite directions (see "add / sub / reduce" below).
struct FqP {
    static constexpr bool kAsmMul = true;
    static constexpr bool kChainAddSub = true;
    FF_HD static constexpr uint32_t mod(int i) {
        constexpr uint32_t M[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u,
                                   0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
        return M[i];
    }
    FF_HD static constexpr uint32_t inv() { return 0xe4866389u; }
    FF_HD static constexpr uint32_t r2(int i) {
        constexpr uint32_t M[8] = {0x538afa89u, 0xf32cfc5bu, 0xd44501fbu, 0xb5e71911u,
                                   0x0a417ff6u, 0x47ab1effu, 0xcab8351fu, 0x06d89f71u};
        return M[i];
    }
    FF_HD static constexpr uint32_t one(int i) {
        constexpr uint32_t M[8] = {0xc58f0d9du, 0xd35d438du, 0xf5c70b3du, 0x0a78eb28u,
                                   0x7879462cu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u};
        return M[i];
    }
};
struct FrP {
    static constexpr bool kAsmMul = true;
    static constexpr bool kChainAddSub = false;
    FF_HD static constexpr uint32_t mod(int i) {
        constexpr uint32_t M[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u,
                                   0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
        return M[i];
    }
    FF_HD static constexpr uint32_t inv() { return 0xefffffffu; }
    FF_HD static constexpr uint32_t r2(int i) {
        constexpr uint32_t M[8] = {0xae216da7u, 0x1bb8e645u, 0xe35c59e3u, 0x53fe3ab1u,
                                   0x53bb8085u, 0x8c49833du, 0x7f4e44a5u, 0x0216d0b1u};
        return M[i];
    }
    FF_HD static constexpr uint32_t one(int i) {
        constexpr uint32_t M[8] = {0x4ffffffbu, 0xac96341cu, 0x9f60cd29u, 0x36fc7695u,
                                   0x7879462eu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u};
        return M[i];
    }
};
// Fr with the compiled CIOS multiply on the device too, for the kernels that
// measured faster with it (ntt.hip, gate.hip).
struct FrCios : FrP {
    static constexpr bool kAsmMul = false;
    static constexpr bool kChainAddSub = false;
};

// ---- generic ops ------------------------------------------------------------
template <class C> FF_HD void ff_set_one(fp256& o) {
    for (int i = 0; i < 8; i++) o.l[i] = C::one(i);
}
FF_HD void ff_set_zero(fp256& o) {
    for (int i = 0; i < 8; i++) o.l[i] = 0;
}
FF_HD bool ff_is_zero(const fp256& a) {
    uint32_t x = 0;
    for (int i = 0; i < 8; i++) x |= a.l[i];
    return x == 0;
}
FF_HD bool ff_eq(const fp256& a, const fp256& b) {
    uint32_t x = 0;
    for (int i = 0; i < 8; i++) x |= a.l[i] ^ b.l[i];
    return x == 0;
}
template <class C> FF_HD bool ff_geq_mod(const fp256& a) {
    for (int i = 7; i >= 0; i--) {
        if (a.l[i] != C::mod(i)) return a.l[i] > C::mod(i);
    }
    return true;
}
// o = a - b, returns borrow
FF_HD uint32_t ff_sub_raw(fp256& o, const fp256& a, const fp256& b) {
    uint64_t brw = 0;
    for (int i = 0; i < 8; i++) {
        uint64_t d = (uint64_t)a.l[i] - b.l[i] - brw;
        o.l[i] = (uint32_t)d;
        brw = (d >> 32) & 1;
    }
    return (uint32_t)brw;
}
FF_HD uint32_t ff_add_raw(fp256& o, const fp256& a, const fp256& b) {
    uint64_t c = 0;
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)a.l[i] + b.l[i];
        o.l[i] = (uint32_t)c;
        c >>= 32;
    }
    return (uint32_t)c;
}
// ---- add / sub / reduce -----------------------------------------------------
// Two forms, chosen by C::kChainAddSub, that return the same bytes.
// The 64-bit form compiles on gfx950 to v_sub_co + v_subb_co + v_ashrrev +
// v_mov + v_lshl_add_u64 per limb and puts the correction behind a branch; the
// borrow differs per lane, so a wave issues both sides: ff_sub<Fq> is about 75
// issue slots. The chain form is v_sub_co / v_subb_co once per limb and the
// correction added under a mask, about 24. In the point formulas of the MSM
// kernels (Fq) that is a third of all vector instructions and frees about 50
// VGPRs (profiles/field_chain_kernel_resources.txt). The NTT and gate kernels
// (FrCios) go the other way under the chain form, to 128 VGPRs and scratch,
// so they keep the 64-bit form.
FF_HD uint32_t ff_adc_(uint32_t a, uint32_t b, uint32_t& carry) {
#if defined(__has_builtin) && __has_builtin(__builtin_addc)
    unsigned out;
    const uint32_t r = __builtin_addc(a, b, carry, &out);
    carry = out;
    return r;
#else
    const uint64_t s = (uint64_t)a + b + carry;
    carry = (uint32_t)(s >> 32);
    return (uint32_t)s;
#endif
}
FF_HD uint32_t ff_sbb_(uint32_t a, uint32_t b, uint32_t& borrow) {
#if defined(__has_builtin) && __has_builtin(__builtin_subc)
    unsigned out;
    const uint32_t r = __builtin_subc(a, b, borrow, &out);
    borrow = out;
    return r;
#else
    const uint64_t d = (uint64_t)a - b - borrow;
    borrow = (uint32_t)(d >> 32) & 1;
    return (uint32_t)d;
#endif
}
// o -= m where extra (bit 256 of o) is set or o >= m: a trial subtract, kept
// iff extra || no borrow
template <class C> FF_HD void ff_cond_sub_mod_chain_(fp256& o, uint32_t extra) {
    uint32_t d[8], brw = 0;
    for (int i = 0; i < 8; i++) d[i] = ff_sbb_(o.l[i], C::mod(i), brw);
    const bool keep = extra != 0 || brw == 0;
    for (int i = 0; i < 8; i++) o.l[i] = keep ? d[i] : o.l[i];
}
template <class C> FF_HD void ff_cond_sub_mod(fp256& o, uint32_t extra) {
    if constexpr (C::kChainAddSub) {
        ff_cond_sub_mod_chain_<C>(o, extra);
    } else if (extra || ff_geq_mod<C>(o)) {
        uint64_t brw = 0;
        for (int i = 0; i < 8; i++) {
            uint64_t d = (uint64_t)o.l[i] - C::mod(i) - brw;
            o.l[i] = (uint32_t)d;
            brw = (d >> 32) & 1;
        }
    }
}
template <class C> FF_HD void ff_add(fp256& o, const fp256& a, const fp256& b) {
    if constexpr (C::kChainAddSub) {
        uint32_t c = 0;
        for (int i = 0; i < 8; i++) o.l[i] = ff_adc_(a.l[i], b.l[i], c);
        ff_cond_sub_mod_chain_<C>(o, c);
    } else {
        uint32_t c = ff_add_raw(o, a, b);
        ff_cond_sub_mod<C>(o, c);
    }
}
template <class C> FF_HD void ff_sub(fp256& o, const fp256& a, const fp256& b) {
    if constexpr (C::kChainAddSub) {
        uint32_t brw = 0;
        for (int i = 0; i < 8; i++) o.l[i] = ff_sbb_(a.l[i], b.l[i], brw);
        const uint32_t mask = 0u - brw;  // add m back iff the chain borrowed
        uint32_t c = 0;
        for (int i = 0; i < 8; i++) o.l[i] = ff_adc_(o.l[i], C::mod(i) & mask, c);
    } else if (ff_sub_raw(o, a, b)) {
        uint64_t c = 0;
        for (int i = 0; i < 8; i++) {
            c += (uint64_t)o.l[i] + C::mod(i);
            o.l[i] = (uint32_t)c;
            c >>= 32;
        }
    }
}
template <class C> FF_HD void ff_neg(fp256& o, const fp256& a) {
    if constexpr (C::kChainAddSub) {  // 0 - a, branch-free like ff_sub
        fp256 z;
        ff_set_zero(z);
        ff_sub<C>(o, z, a);
        return;
    }
    if (ff_is_zero(a)) { o = a; return; }
    fp256 m;
    for (int i = 0; i < 8; i++) m.l[i] = C::mod(i);
    ff_sub_raw(o, m, a);
}

// CIOS Montgomery multiplication, 8x32 limbs, 64-bit accumulators: the host
// multiply, and the device multiply of the fields with kAsmMul == false. The
// asm column form below must stay bit-identical to this.
template <class C> FF_HD void ff_mul_cios(fp256& o, const fp256& a, const fp256& b) {
    uint32_t t[10];
    for (int i = 0; i < 10; i++) t[i] = 0;
    for (int i = 0; i < 8; i++) {
        uint64_t cc = 0;
        const uint32_t ai = a.l[i];
        for (int j = 0; j < 8; j++) {
            uint64_t x = (uint64_t)ai * b.l[j] + t[j] + (uint32_t)cc;
            t[j] = (uint32_t)x;
            cc = x >> 32;
        }
        uint64_t x = (uint64_t)t[8] + (uint32_t)cc;
        t[8] = (uint32_t)x;
        t[9] = (uint32_t)(x >> 32);
        const uint32_t m = t[0] * C::inv();
        uint64_t x2 = (uint64_t)m * C::mod(0) + t[0];
        cc = x2 >> 32;
        for (int j = 1; j < 8; j++) {
            x2 = (uint64_t)m * C::mod(j) + t[j] + (uint32_t)cc;
            t[j - 1] = (uint32_t)x2;
            cc = x2 >> 32;
        }
        x2 = (uint64_t)t[8] + (uint32_t)cc;
        t[7] = (uint32_t)x2;
        t[8] = t[9] + (uint32_t)(x2 >> 32);
    }
    for (int i = 0; i < 8; i++) o.l[i] = t[i];
    ff_cond_sub_mod<C>(o, t[8]);
}
// ---- device multiply: hand-scheduled column Montgomery --------------------
// On gfx950 the asm column form runs at ~135 G Fq-mul/s vs ~103 for the
// compiled CIOS (measured, tools/microbench.hip) and is bit-identical
// (256K-lane chained check + the whole GPU parity suite). A field takes it
// through C::kAsmMul; building everything with -DSPECTRE_NO_ASM_MUL turns it
// off for every field (debugging / A-B).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(SPECTRE_NO_ASM_MUL)
#define FF_HAVE_ASM_MUL 1
#endif

#if defined(FF_HAVE_ASM_MUL)
// Single product: acc += a*b (64-bit mad), ovf += carry-out. Explicit
// carry-mask pairs ("=s"): a vcc clobber makes hipcc pad every block
// boundary with s_nop hazards.
// MEASURED NEGATIVE RESULT (r2): fusing 2/4 products per asm block to cut
// those boundary s_nops produces WRONG results at full-range operands — a
// v_mad_u64_u32 reading the 64-bit acc written by a mad one instruction
// earlier needs >= 2 intervening issue slots (the compiler's conservative
// inter-block s_nop was supplying exactly that); and the s_nops are hidden
// by co-resident waves anyway (grouped rate unchanged at 135 G/s). Keep
// one mad+addc pair per block.
__device__ __forceinline__ void ff_mad64_(uint64_t& acc, uint32_t& ovf,
                                          uint32_t a, uint32_t b) {
    uint64_t c;
    asm volatile("v_mad_u64_u32 %0, %2, %3, %4, %0\n\t"
                 "v_addc_co_u32 %1, %2, 0, %1, %2"
                 : "+v"(acc), "+v"(ovf), "=s"(c)
                 : "v"(a), "v"(b));
}
__device__ __forceinline__ void ff_mad64_s_(uint64_t& acc, uint32_t& ovf,
                                            uint32_t a, uint32_t b_uniform) {
    uint64_t c;
    asm volatile("v_mad_u64_u32 %0, %2, %3, %4, %0\n\t"
                 "v_addc_co_u32 %1, %2, 0, %1, %2"
                 : "+v"(acc), "+v"(ovf), "=s"(c)
                 : "v"(a), "s"(b_uniform));
}
template <class C, int K>
__device__ __forceinline__ void detail_ff_low_cols(uint64_t& acc,
                                                   uint32_t& ovf,
                                                   const uint32_t* a,
                                                   const uint32_t* b,
                                                   uint32_t* m) {
    if constexpr (K < 8) {
#pragma unroll
        for (int i = 0; i <= K; i++) ff_mad64_(acc, ovf, a[i], b[K - i]);
#pragma unroll
        for (int i = 0; i < K; i++) ff_mad64_s_(acc, ovf, m[i], C::mod(K - i));
        m[K] = (uint32_t)acc * C::inv();
        ff_mad64_s_(acc, ovf, m[K], C::mod(0));
        acc = (acc >> 32) | ((uint64_t)ovf << 32);
        ovf = 0;
        detail_ff_low_cols<C, K + 1>(acc, ovf, a, b, m);
    }
}
template <class C, int K>
__device__ __forceinline__ void detail_ff_high_cols(uint64_t& acc,
                                                    uint32_t& ovf,
                                                    const uint32_t* a,
                                                    const uint32_t* b,
                                                    const uint32_t* m,
                                                    uint32_t* out) {
    if constexpr (K < 15) {
#pragma unroll
        for (int i = K - 7; i < 8; i++) ff_mad64_(acc, ovf, a[i], b[K - i]);
#pragma unroll
        for (int i = K - 7; i < 8; i++) ff_mad64_s_(acc, ovf, m[i], C::mod(K - i));
        out[K - 8] = (uint32_t)acc;
        acc = (acc >> 32) | ((uint64_t)ovf << 32);
        ovf = 0;
        detail_ff_high_cols<C, K + 1>(acc, ovf, a, b, m, out);
    }
}
// Product-scanning Montgomery: low columns annihilated with m_k as they
// complete, high columns emit the result; ovf counts 64-bit carry-outs per
// column (<= 16 products). Result < 2p, one conditional subtract.
template <class C>
__device__ __forceinline__ void ff_mul_cols(fp256& o, const fp256& A,
                                            const fp256& B) {
    uint32_t m[8];
    uint64_t acc = 0;
    uint32_t ovf = 0;
    detail_ff_low_cols<C, 0>(acc, ovf, A.l, B.l, m);
    detail_ff_high_cols<C, 8>(acc, ovf, A.l, B.l, m, o.l);
    o.l[7] = (uint32_t)acc;
    // bits >= 256 provably zero (result < 2p < 2^255); high half passed to
    // the conditional subtract so a violated precondition reduces loudly
    // rather than truncating silently.
    ff_cond_sub_mod<C>(o, (uint32_t)(acc >> 32));
}

// ---- device squaring: the column form with 36 products instead of 64 -------
// With B = 2^32 and T_i = sum_{j>i} a_j B^j,
//   a^2 = sum_i a_i^2 B^(2i) + sum_i a_i (2 T_i).
// 2 T_i has the limbs D(i,j), j = i+1 .. 7:
//   D(i,j)   = (a_j << 1) | (a_(j-1) >> 31)   for j > i + 1   (dbl[j])
//   D(i,i+1) =  a_(i+1) << 1                                  (adj[i+1])
// adj has its low bit clear because limb i is not part of T_i, and nothing is
// lost at the top while a < 2^255 (a_7 >> 31 == 0): true of every reduced
// element of a field whose modulus is below 2^255, false at 2^256 - 1. Column
// K gets a_i D(i, K-i) for 2i < K and a_(K/2)^2 for even K; the m_k products,
// the (acc, ovf) scheme and the one-product asm blocks are those of
// ff_mul_cols, and so are the result bytes.
template <int K>
__device__ __forceinline__ void detail_ff_sqr_col(uint64_t& acc, uint32_t& ovf,
                                                  const uint32_t* a,
                                                  const uint32_t* adj,
                                                  const uint32_t* dbl) {
#pragma unroll
    for (int i = K < 8 ? 0 : K - 7; 2 * i + 1 < K; i++)
        ff_mad64_(acc, ovf, a[i], dbl[K - i]);
    if constexpr (K % 2) ff_mad64_(acc, ovf, a[K / 2], adj[K / 2 + 1]);
    else ff_mad64_(acc, ovf, a[K / 2], a[K / 2]);
}
template <class C, int K>
__device__ __forceinline__ void detail_ff_sqr_low_cols(uint64_t& acc,
                                                       uint32_t& ovf,
                                                       const uint32_t* a,
                                                       const uint32_t* adj,
                                                       const uint32_t* dbl,
                                                       uint32_t* m) {
    if constexpr (K < 8) {
        detail_ff_sqr_col<K>(acc, ovf, a, adj, dbl);
#pragma unroll
        for (int i = 0; i < K; i++) ff_mad64_s_(acc, ovf, m[i], C::mod(K - i));
        m[K] = (uint32_t)acc * C::inv();
        ff_mad64_s_(acc, ovf, m[K], C::mod(0));
        acc = (acc >> 32) | ((uint64_t)ovf << 32);
        ovf = 0;
        detail_ff_sqr_low_cols<C, K + 1>(acc, ovf, a, adj, dbl, m);
    }
}
template <class C, int K>
__device__ __forceinline__ void detail_ff_sqr_high_cols(uint64_t& acc,
                                                        uint32_t& ovf,
                                                        const uint32_t* a,
                                                        const uint32_t* adj,
                                                        const uint32_t* dbl,
                                                        const uint32_t* m,
                                                        uint32_t* out) {
    if constexpr (K < 15) {
        detail_ff_sqr_col<K>(acc, ovf, a, adj, dbl);
#pragma unroll
        for (int i = K - 7; i < 8; i++) ff_mad64_s_(acc, ovf, m[i], C::mod(K - i));
        out[K - 8] = (uint32_t)acc;
        acc = (acc >> 32) | ((uint64_t)ovf << 32);
        ovf = 0;
        detail_ff_sqr_high_cols<C, K + 1>(acc, ovf, a, adj, dbl, m, out);
    }
}
template <class C>
__device__ __forceinline__ void ff_sqr_cols(fp256& o, const fp256& A) {
    static_assert(C::mod(7) < 0x80000000u,
                  "the doubled limbs drop bit 255: reduced elements must be "
                  "below 2^255");
    uint32_t a[8], adj[8], dbl[8], m[8];
#pragma unroll
    for (int i = 0; i < 8; i++) a[i] = A.l[i];  // o may be A
    adj[0] = dbl[0] = 0;                        // never read
#pragma unroll
    for (int j = 1; j < 8; j++) {
        adj[j] = a[j] << 1;
        dbl[j] = (a[j] << 1) | (a[j - 1] >> 31);
    }
    uint64_t acc = 0;
    uint32_t ovf = 0;
    detail_ff_sqr_low_cols<C, 0>(acc, ovf, a, adj, dbl, m);
    detail_ff_sqr_high_cols<C, 8>(acc, ovf, a, adj, dbl, m, o.l);
    o.l[7] = (uint32_t)acc;
    ff_cond_sub_mod<C>(o, (uint32_t)(acc >> 32));
}

// ---- device sum of two products: one reduction for a*b + c*d ---------------
// The column form with a second operand pair feeding each column: 128
// operand products and 64 m*p products, where two multiplies pay 2*(64 + 64).
// a*b + c*d < 2 m^2, so the value after the m_k products is below
// m (2m / 2^256 + 1), which is below 2m (and below 2^255) while m < 2^255:
// the one trial subtract is enough and the bytes are those of
// ff_add(ff_mul(a, b), ff_mul(c, d)). A column takes at most 16 + 8 products.
template <class C, int K>
__device__ __forceinline__ void detail_ff_dot2_low_cols(
    uint64_t& acc, uint32_t& ovf, const uint32_t* a, const uint32_t* b,
    const uint32_t* c, const uint32_t* d, uint32_t* m) {
    if constexpr (K < 8) {
#pragma unroll
        for (int i = 0; i <= K; i++) {
            ff_mad64_(acc, ovf, a[i], b[K - i]);
            ff_mad64_(acc, ovf, c[i], d[K - i]);
        }
#pragma unroll
        for (int i = 0; i < K; i++) ff_mad64_s_(acc, ovf, m[i], C::mod(K - i));
        m[K] = (uint32_t)acc * C::inv();
        ff_mad64_s_(acc, ovf, m[K], C::mod(0));
        acc = (acc >> 32) | ((uint64_t)ovf << 32);
        ovf = 0;
        detail_ff_dot2_low_cols<C, K + 1>(acc, ovf, a, b, c, d, m);
    }
}
template <class C, int K>
__device__ __forceinline__ void detail_ff_dot2_high_cols(
    uint64_t& acc, uint32_t& ovf, const uint32_t* a, const uint32_t* b,
    const uint32_t* c, const uint32_t* d, const uint32_t* m, uint32_t* out) {
    if constexpr (K < 15) {
#pragma unroll
        for (int i = K - 7; i < 8; i++) {
            ff_mad64_(acc, ovf, a[i], b[K - i]);
            ff_mad64_(acc, ovf, c[i], d[K - i]);
        }
#pragma unroll
        for (int i = K - 7; i < 8; i++) ff_mad64_s_(acc, ovf, m[i], C::mod(K - i));
        out[K - 8] = (uint32_t)acc;
        acc = (acc >> 32) | ((uint64_t)ovf << 32);
        ovf = 0;
        detail_ff_dot2_high_cols<C, K + 1>(acc, ovf, a, b, c, d, m, out);
    }
}
template <class C>
__device__ __forceinline__ void ff_dot2_cols(fp256& o, const fp256& A,
                                             const fp256& B, const fp256& Cc,
                                             const fp256& D) {
    static_assert(C::mod(7) < 0x80000000u,
                  "one trial subtract after a*b + c*d needs 2m <= 2^256");
    uint32_t m[8];
    uint64_t acc = 0;
    uint32_t ovf = 0;
    detail_ff_dot2_low_cols<C, 0>(acc, ovf, A.l, B.l, Cc.l, D.l, m);
    detail_ff_dot2_high_cols<C, 8>(acc, ovf, A.l, B.l, Cc.l, D.l, m, o.l);
    o.l[7] = (uint32_t)acc;
    ff_cond_sub_mod<C>(o, (uint32_t)(acc >> 32));
}
#endif

// The one multiply: the form the field names on the device, CIOS on the host.
template <class C> FF_HD void ff_mul(fp256& o, const fp256& a, const fp256& b) {
#if defined(FF_HAVE_ASM_MUL)
    if constexpr (C::kAsmMul) {
        ff_mul_cols<C>(o, a, b);
        return;
    }
#endif
    ff_mul_cios<C>(o, a, b);
}

// The one squaring: where the field multiplies with the asm column form, the
// column squaring; ff_mul(a, a) elsewhere. a must be reduced (a < m).
template <class C> FF_HD void ff_sqr(fp256& o, const fp256& a) {
#if defined(FF_HAVE_ASM_MUL)
    if constexpr (C::kAsmMul) {
        ff_sqr_cols<C>(o, a);
        return;
    }
#endif
    ff_mul<C>(o, a, a);
}

// o = a*b + c*d (Montgomery), canonical: the bytes of
// ff_add(ff_mul(a, b), ff_mul(c, d)) with one reduction where the field
// multiplies with the asm column form. o may be any of the operands.
template <class C>
FF_HD void ff_dot2(fp256& o, const fp256& a, const fp256& b, const fp256& c,
                   const fp256& d) {
#if defined(FF_HAVE_ASM_MUL)
    if constexpr (C::kAsmMul) {
        ff_dot2_cols<C>(o, a, b, c, d);
        return;
    }
#endif
    fp256 t;
    ff_mul<C>(t, a, b);
    ff_mul<C>(o, c, d);
    ff_add<C>(o, t, o);
}

// Montgomery conversion
template <class C> FF_HD void ff_to_mont(fp256& o, const fp256& a_canon) {
    fp256 r2;
    for (int i = 0; i < 8; i++) r2.l[i] = C::r2(i);
    ff_mul<C>(o, a_canon, r2);
}
template <class C> FF_HD void ff_from_mont(fp256& o, const fp256& a) {
    fp256 one;
    ff_set_zero(one);
    one.l[0] = 1;
    ff_mul<C>(o, a, one);
}

// a^e for small 32-bit exponent (twiddle powers)
template <class C> FF_HD void ff_pow_u32(fp256& o, const fp256& a, uint32_t e) {
    fp256 acc, base = a;
    ff_set_one<C>(acc);
    while (e) {
        if (e & 1) ff_mul<C>(acc, acc, base);
        e >>= 1;
        if (e) ff_sqr<C>(base, base);
    }
    o = acc;
}
// Fermat inverse a^(m-2), square-and-multiply over the exponent's 8 words.
// The words are selected by compares, not read from a local array, which the
// device compiler would place in scratch memory; the loops stay rolled. In a
// kernel every branch is uniform when the wave inverts one value.
template <class C> FF_HD void ff_inv(fp256& o, const fp256& a) {
    static_assert(C::mod(0) >= 2u, "m - 2 must not borrow out of the low word");
    fp256 acc, base = a;
    ff_set_one<C>(acc);
#pragma unroll 1
    for (uint32_t w = 0; w < 8; w++) {
        uint32_t bits = C::mod(0) - 2u;
#pragma unroll
        for (uint32_t i = 1; i < 8; i++) bits = w == i ? C::mod(i) : bits;
#pragma unroll 1
        for (uint32_t b = 0; b < 32; b++) {
            if ((bits >> b) & 1) ff_mul<C>(acc, acc, base);
            ff_sqr<C>(base, base);
        }
    }
    o = acc;
}

FF_HD void ff_from_bytes(fp256& o, const uint8_t* b) { memcpy(o.l, b, 32); }
FF_HD void ff_to_bytes(uint8_t* b, const fp256& a) { memcpy(b, a.l, 32); }

using Fq = FqP;
using Fr = FrP;

// ---- split LDS element ------------------------------------------------------
// A 32-B element kept whole in LDS spans 8 banks, so power-of-two strides
// conflict. The kernels store it as two 16-B halves, the low one at lds4[lo]
// and the high one `dist` entries further on: consecutive elements then
// stride 4 banks. The caller owns the layout (lo and dist). The sum is written
// dist + lo, the order under which k_ntt_pass was measured (the other order
// compiles to different code, profiles/field_layer_text_identity.txt).
#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void lds_split_ld(const uint4* lds4, uint32_t lo,
                                             uint32_t dist, fp256& o) {
    uint4 l = lds4[lo], h = lds4[dist + lo];
    memcpy(&o.l[0], &l, 16);
    memcpy(&o.l[4], &h, 16);
}
__device__ __forceinline__ void lds_split_st(uint4* lds4, uint32_t lo,
                                             uint32_t dist, const fp256& v) {
    uint4 l, h;
    memcpy(&l, &v.l[0], 16);
    memcpy(&h, &v.l[4], 16);
    lds4[lo] = l;
    lds4[dist + lo] = h;
}
#endif
