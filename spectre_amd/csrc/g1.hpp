// g1.hpp — BN254 G1 point arithmetic (Jacobian and XYZZ over Fq), host +
// device.
//
// PRODUCT CODE. Jacobian formulas (the host fold and finish, the 96-byte
// interface): EFD dbl-2009-l (a=0), madd-2007-bl, add-2007-bl with explicit
// degenerate-case handling. Jacobian identity: Z == 0. The XYZZ forms below
// them are what the MSM kernels add with. In the additions of both (and in
// the XYZZ doubling), Y3 = r*(V - X3) - c*J is
// one ff_dot2: two products under one Montgomery reduction.
// Affine memory image = halo2curves G1Affine: x||y Montgomery Fq, 64 bytes,
// identity encoded as (0, 0) (x=y=0 is not on y^2 = x^3 + 3).
//
// The accumulate primitives (g1j_dbl_ip / g1j_madd_ip / g1j_add_ip) mutate
// their accumulator in place: on gfx950 a g1_jac is 24 VGPRs, and the
// copy-in/copy-out style (o, p, q all distinct) makes hipcc spill to scratch
// in the MSM kernels — the in-place forms keep the whole working set in
// registers.
#pragma once
#include "ff.hpp"

struct g1_affine {
    fp256 x, y;  // Montgomery Fq; identity iff x==0 && y==0
};
struct g1_jac {
    fp256 X, Y, Z;  // identity iff Z==0
};

FF_HD bool g1a_is_inf(const g1_affine& p) { return ff_is_zero(p.x) && ff_is_zero(p.y); }
FF_HD void g1j_set_inf(g1_jac& p) {
    ff_set_one<Fq>(p.X);
    ff_set_one<Fq>(p.Y);
    ff_set_zero(p.Z);
}
FF_HD bool g1j_is_inf(const g1_jac& p) { return ff_is_zero(p.Z); }
FF_HD void g1j_from_affine(g1_jac& o, const g1_affine& p) {
    if (g1a_is_inf(p)) { g1j_set_inf(o); return; }
    o.X = p.x;
    o.Y = p.y;
    ff_set_one<Fq>(o.Z);
}

// p = 2p, dbl-2009-l (a = 0), in place
FF_HD void g1j_dbl_ip(g1_jac& p) {
    if (g1j_is_inf(p)) return;
    fp256 A, B, C, D, E, F;
    ff_sqr<Fq>(A, p.X);
    ff_sqr<Fq>(B, p.Y);
    ff_sqr<Fq>(C, B);
    ff_add<Fq>(D, p.X, B);
    ff_sqr<Fq>(D, D);
    ff_sub<Fq>(D, D, A);
    ff_sub<Fq>(D, D, C);
    ff_add<Fq>(D, D, D);
    ff_add<Fq>(E, A, A);
    ff_add<Fq>(E, E, A);
    ff_sqr<Fq>(F, E);
    ff_mul<Fq>(p.Z, p.Y, p.Z);
    ff_add<Fq>(p.Z, p.Z, p.Z);
    ff_sub<Fq>(p.X, F, D);
    ff_sub<Fq>(p.X, p.X, D);
    ff_sub<Fq>(D, D, p.X);
    ff_mul<Fq>(D, E, D);
    ff_add<Fq>(C, C, C);
    ff_add<Fq>(C, C, C);
    ff_add<Fq>(C, C, C);
    ff_sub<Fq>(p.Y, D, C);
}

// p += q (q affine), madd-2007-bl, in place
FF_HD void g1j_madd_ip(g1_jac& p, const g1_affine& q) {
    if (g1a_is_inf(q)) return;
    if (g1j_is_inf(p)) { g1j_from_affine(p, q); return; }
    fp256 Z1Z1, U2, S2, H, HH, I, J, rr, V;
    ff_sqr<Fq>(Z1Z1, p.Z);
    ff_mul<Fq>(U2, q.x, Z1Z1);
    ff_mul<Fq>(S2, q.y, p.Z);
    ff_mul<Fq>(S2, S2, Z1Z1);
    ff_sub<Fq>(H, U2, p.X);
    ff_sub<Fq>(rr, S2, p.Y);
    if (ff_is_zero(H)) {
        if (ff_is_zero(rr)) { g1j_dbl_ip(p); return; }
        g1j_set_inf(p);
        return;
    }
    ff_add<Fq>(rr, rr, rr);
    ff_sqr<Fq>(HH, H);
    ff_add<Fq>(I, HH, HH);
    ff_add<Fq>(I, I, I);
    ff_mul<Fq>(J, H, I);
    ff_mul<Fq>(V, p.X, I);
    // Z3 = (Z1+H)^2 - Z1Z1 - HH   (consumes p.Z, H, Z1Z1, HH)
    ff_add<Fq>(p.Z, p.Z, H);
    ff_sqr<Fq>(p.Z, p.Z);
    ff_sub<Fq>(p.Z, p.Z, Z1Z1);
    ff_sub<Fq>(p.Z, p.Z, HH);
    // X3 = rr^2 - J - 2V
    ff_sqr<Fq>(H, rr);  // reuse H
    ff_sub<Fq>(H, H, J);
    ff_sub<Fq>(H, H, V);
    ff_sub<Fq>(H, H, V);
    // Y3 = rr*(V - X3) + (-2*Y1)*J, one reduction
    ff_sub<Fq>(V, V, H);
    ff_add<Fq>(p.Y, p.Y, p.Y);
    ff_neg<Fq>(p.Y, p.Y);
    ff_dot2<Fq>(p.Y, rr, V, p.Y, J);
    p.X = H;
}

// p += q (both Jacobian), add-2007-bl, in place
FF_HD void g1j_add_ip(g1_jac& p, const g1_jac& q) {
    if (g1j_is_inf(q)) return;
    if (g1j_is_inf(p)) { p = q; return; }
    fp256 Z1Z1, Z2Z2, U1, U2, S1, S2, H, I, J, rr, V;
    ff_sqr<Fq>(Z1Z1, p.Z);
    ff_sqr<Fq>(Z2Z2, q.Z);
    ff_mul<Fq>(U1, p.X, Z2Z2);
    ff_mul<Fq>(U2, q.X, Z1Z1);
    ff_mul<Fq>(S1, p.Y, q.Z);
    ff_mul<Fq>(S1, S1, Z2Z2);
    ff_mul<Fq>(S2, q.Y, p.Z);
    ff_mul<Fq>(S2, S2, Z1Z1);
    ff_sub<Fq>(H, U2, U1);
    ff_sub<Fq>(rr, S2, S1);
    if (ff_is_zero(H)) {
        if (ff_is_zero(rr)) { g1j_dbl_ip(p); return; }
        g1j_set_inf(p);
        return;
    }
    ff_add<Fq>(rr, rr, rr);
    ff_add<Fq>(I, H, H);
    ff_sqr<Fq>(I, I);
    ff_mul<Fq>(J, H, I);
    ff_mul<Fq>(V, U1, I);
    // Z3 = ((Z1+Z2)^2 - Z1Z1 - Z2Z2) * H
    ff_add<Fq>(p.Z, p.Z, q.Z);
    ff_sqr<Fq>(p.Z, p.Z);
    ff_sub<Fq>(p.Z, p.Z, Z1Z1);
    ff_sub<Fq>(p.Z, p.Z, Z2Z2);
    ff_mul<Fq>(p.Z, p.Z, H);
    // X3 = rr^2 - J - 2V
    ff_sqr<Fq>(H, rr);
    ff_sub<Fq>(H, H, J);
    ff_sub<Fq>(H, H, V);
    ff_sub<Fq>(H, H, V);
    // Y3 = rr*(V - X3) + (-2*S1)*J, one reduction
    ff_sub<Fq>(V, V, H);
    ff_add<Fq>(S1, S1, S1);
    ff_neg<Fq>(S1, S1);
    ff_dot2<Fq>(p.Y, rr, V, S1, J);
    p.X = H;
}

// ---- XYZZ: x = X/ZZ, y = Y/ZZZ, ZZ^3 == ZZZ^2; identity iff ZZ == 0 ---------
// The coordinates of the MSM kernels from the bucket accumulator to the
// window partials (msm.hip). EFD mADD-2008-s (8M + 2S), add-2008-s (12M + 2S)
// and dbl-2008-s-1, with Y3 = R*(Q - X3) + (-c)*PPP through ff_dot2. The
// degenerate cases are handled as in the Jacobian forms above.
struct g1_xyzz {
    fp256 X, Y, ZZ, ZZZ;
};
FF_HD void g1x_set_inf(g1_xyzz& p) {
    ff_set_one<Fq>(p.X);
    ff_set_one<Fq>(p.Y);
    ff_set_zero(p.ZZ);
    ff_set_zero(p.ZZZ);
}
FF_HD bool g1x_is_inf(const g1_xyzz& p) { return ff_is_zero(p.ZZ); }
FF_HD void g1x_from_affine(g1_xyzz& o, const g1_affine& p) {
    if (g1a_is_inf(p)) { g1x_set_inf(o); return; }
    o.X = p.x;
    o.Y = p.y;
    ff_set_one<Fq>(o.ZZ);
    ff_set_one<Fq>(o.ZZZ);
}

// p = 2p, dbl-2008-s-1, in place
FF_HD void g1x_dbl_ip(g1_xyzz& p) {
    if (g1x_is_inf(p)) return;
    fp256 U, V, W, S, M;
    ff_add<Fq>(U, p.Y, p.Y);
    ff_sqr<Fq>(V, U);
    ff_mul<Fq>(W, U, V);
    ff_mul<Fq>(S, p.X, V);
    ff_sqr<Fq>(M, p.X);
    ff_add<Fq>(U, M, M);
    ff_add<Fq>(M, U, M);
    ff_mul<Fq>(p.ZZ, V, p.ZZ);
    ff_mul<Fq>(p.ZZZ, W, p.ZZZ);
    // X3 = M^2 - 2S
    ff_sqr<Fq>(p.X, M);
    ff_sub<Fq>(p.X, p.X, S);
    ff_sub<Fq>(p.X, p.X, S);
    // Y3 = M*(S - X3) + (-Y1)*W, one reduction
    ff_sub<Fq>(S, S, p.X);
    ff_neg<Fq>(p.Y, p.Y);
    ff_dot2<Fq>(p.Y, M, S, p.Y, W);
}

// The part mADD and add share once U1, S1 (the accumulator's side) and
// U2, S2 are known: P = U2 - U1, R = S2 - S1, then X3, Y3 and PP, PPP for the
// caller's ZZ3, ZZZ3. False, with p already set, when P == 0.
FF_HD bool g1x_add_core_(g1_xyzz& p, const fp256& U1, fp256& S1, fp256& U2,
                         fp256& S2, fp256& PP, fp256& PPP) {
    ff_sub<Fq>(U2, U2, U1);  // P
    ff_sub<Fq>(S2, S2, S1);  // R
    if (ff_is_zero(U2)) {
        if (ff_is_zero(S2)) g1x_dbl_ip(p);
        else g1x_set_inf(p);
        return false;
    }
    fp256 Q;
    ff_sqr<Fq>(PP, U2);
    ff_mul<Fq>(PPP, U2, PP);
    ff_mul<Fq>(Q, U1, PP);
    // X3 = R^2 - PPP - 2Q
    ff_sqr<Fq>(p.X, S2);
    ff_sub<Fq>(p.X, p.X, PPP);
    ff_sub<Fq>(p.X, p.X, Q);
    ff_sub<Fq>(p.X, p.X, Q);
    // Y3 = R*(Q - X3) + (-S1)*PPP, one reduction
    ff_sub<Fq>(Q, Q, p.X);
    ff_neg<Fq>(S1, S1);
    ff_dot2<Fq>(p.Y, S2, Q, S1, PPP);
    return true;
}

// p += q (q affine), mADD-2008-s, in place
FF_HD void g1x_madd_ip(g1_xyzz& p, const g1_affine& q) {
    if (g1a_is_inf(q)) return;
    if (g1x_is_inf(p)) { g1x_from_affine(p, q); return; }
    fp256 U1 = p.X, S1 = p.Y, U2, S2, PP, PPP;
    ff_mul<Fq>(U2, q.x, p.ZZ);
    ff_mul<Fq>(S2, q.y, p.ZZZ);
    if (!g1x_add_core_(p, U1, S1, U2, S2, PP, PPP)) return;
    ff_mul<Fq>(p.ZZ, p.ZZ, PP);
    ff_mul<Fq>(p.ZZZ, p.ZZZ, PPP);
}

// p += q (both XYZZ), add-2008-s, in place
FF_HD void g1x_add_ip(g1_xyzz& p, const g1_xyzz& q) {
    if (g1x_is_inf(q)) return;
    if (g1x_is_inf(p)) { p = q; return; }
    fp256 U1, S1, U2, S2, PP, PPP;
    ff_mul<Fq>(U1, p.X, q.ZZ);
    ff_mul<Fq>(S1, p.Y, q.ZZZ);
    ff_mul<Fq>(U2, q.X, p.ZZ);
    ff_mul<Fq>(S2, q.Y, p.ZZZ);
    if (!g1x_add_core_(p, U1, S1, U2, S2, PP, PPP)) return;
    ff_mul<Fq>(p.ZZ, p.ZZ, q.ZZ);
    ff_mul<Fq>(p.ZZ, p.ZZ, PP);
    ff_mul<Fq>(p.ZZZ, p.ZZZ, q.ZZZ);
    ff_mul<Fq>(p.ZZZ, p.ZZZ, PPP);
}

// (X*ZZ^2, Y*ZZZ^2, ZZZ): the same point in Jacobian form, 2M + 2S
FF_HD void g1x_to_jac(g1_jac& o, const g1_xyzz& p) {
    if (g1x_is_inf(p)) { g1j_set_inf(o); return; }
    fp256 t;
    ff_sqr<Fq>(t, p.ZZ);
    ff_mul<Fq>(o.X, p.X, t);
    ff_sqr<Fq>(t, p.ZZZ);
    ff_mul<Fq>(o.Y, p.Y, t);
    o.Z = p.ZZZ;
}

// host-side normalization (field inversion — used once per MSM result)
FF_HD void g1j_to_affine(g1_affine& o, const g1_jac& p) {
    if (g1j_is_inf(p)) {
        ff_set_zero(o.x);
        ff_set_zero(o.y);
        return;
    }
    fp256 zi, zi2, zi3;
    ff_inv<Fq>(zi, p.Z);
    ff_sqr<Fq>(zi2, zi);
    ff_mul<Fq>(zi3, zi2, zi);
    ff_mul<Fq>(o.x, p.X, zi2);
    ff_mul<Fq>(o.y, p.Y, zi3);
}
