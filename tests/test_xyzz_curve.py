"""The XYZZ point forms of g1.hpp (g1x_madd_ip, g1x_add_ip, g1x_dbl_ip,
g1x_to_jac) on the host and on the device, against the bigint curve of
tests/golden/bn254_ref.py, and the Jacobian forms, whose Y3 goes through
ff_dot2, against the bytes their formulas give in bigints.

Points are compared as affine points, and every non-identity XYZZ output must
satisfy ZZ^3 == ZZZ^2 with reduced coordinates (curve_probe_lib.xyzz_to_affine
asserts both). The operands are the curve_cases() / dbl_cases() catalogue of
edge_operands.py, an operand P presented as (lam^2 x, lam^3 y, lam^2, lam^3):
the identity on either side and on both, P + P with ZZ == 1 and ZZ != 1,
P + (-P), generic sums; then a run of mixed additions that doubles at ZZ != 1
(acc = 2P plus affine 2P), cancels to the identity and goes on.
"""
import pytest

import curve_probe_lib as cp
import edge_operands as eo

P, ref = eo.P, eo.ref
ONE = eo.fq_img(1)


# ----------------------------------------------------------------- XYZZ ops
def xyzz_inputs(op):
    """(a bytes, b bytes or None, expected affine results) of an XYZZ op;
    x_add_swapped is x_add with the operands exchanged."""
    if op == "x_dbl":
        cs = eo.dbl_cases()
        return (b"".join(cp.xyzz_bytes(p, lam) for p, lam, _ in cs), None,
                [c[2] for c in cs])
    cs = eo.curve_cases()
    left = b"".join(cp.xyzz_bytes(p, lam) for p, lam, _, _, _ in cs)
    if op == "x_madd":
        right = b"".join(ref.g1_to_bytes(q) for _, _, q, _, _ in cs)
    else:
        right = b"".join(cp.xyzz_bytes(q, lq) for _, _, q, lq, _ in cs)
    if op == "x_add_swapped":
        left, right = right, left
    return left, right, [c[4] for c in cs]


def jac_inputs(op):
    """The same operands for the Jacobian form of the same op."""
    if op == "x_dbl":
        return (b"".join(eo.jac_bytes(p, lam) for p, lam, _ in eo.dbl_cases()),
                None)
    cs = eo.curve_cases()
    left = b"".join(eo.jac_bytes(p, lam) for p, lam, _, _, _ in cs)
    if op == "x_madd":
        right = b"".join(ref.g1_to_bytes(q) for _, _, q, _, _ in cs)
    else:
        right = b"".join(eo.jac_bytes(q, lq) for _, _, q, lq, _ in cs)
    if op == "x_add_swapped":
        left, right = right, left
    return left, right


XYZZ_OPS = ["x_dbl", "x_madd", "x_add", "x_add_swapped"]
JAC_OF = {"x_dbl": "g1_dbl", "x_madd": "g1_madd", "x_add": "g1_add",
          "x_add_swapped": "g1_add"}


def check_xyzz(where, op) -> bytes:
    a, b, want = xyzz_inputs(op)
    n = len(want)
    out = cp.curve_call(where, op.replace("_swapped", ""), "Fq", a, b, 128, n)
    for i in range(n):
        got = cp.xyzz_to_affine(out[128 * i:128 * (i + 1)])
        assert got == want[i], (
            f"{where} {op} case {i}\n  got  {eo.desc_point(got)}\n"
            f"  want {eo.desc_point(want[i])}")
    # g1x_to_jac of each result: a Jacobian image of the same point, and the
    # point the Jacobian form of the op gives from the same operands
    jac = cp.curve_call(where, "x_to_jac", "Fq", out, None, 96, n)
    ja, jb = jac_inputs(op)
    jref = cp.field_call(where, JAC_OF[op], "Fq", ja, jb, 96, n)
    for i in range(n):
        got = eo.jac_to_affine(jac[96 * i:96 * (i + 1)])
        assert got == want[i], f"{where} {op} case {i}: g1x_to_jac"
        assert got == eo.jac_to_affine(jref[96 * i:96 * (i + 1)]), (
            f"{where} {op} case {i}: g1x_to_jac against {JAC_OF[op]}")
        if got is None:  # the identity maps to the Jacobian identity's bytes
            assert jac[96 * i:96 * (i + 1)] == eo.imgs_bytes([ONE, ONE, 0])
    return out


def check_run(where):
    """One accumulator through mixed additions, every step checked: from the
    identity, P, P again (doubles at ZZ == 1), 2P (doubles at ZZ != 1), Q,
    -(4P + Q) (cancels to the identity in mid-run), Q, -Q (the identity
    again, at ZZ == 1), P."""
    pts = eo.edge_points()
    p, q = pts[1], pts[2]
    p2 = ref.g1_add(p, p)
    p4q = ref.g1_add(ref.g1_add(p2, p2), q)
    steps = [p, p, p2, q, ref.g1_neg(p4q), q, ref.g1_neg(q), p]
    acc, want = cp.xyzz_bytes(None, 1), None
    seen_inf = seen_zz = 0
    for i, s in enumerate(steps):
        if want is not None and want == s:
            seen_zz += eo.imgs_from(acc)[2] != ONE
        acc = cp.curve_call(where, "x_madd", "Fq", acc, ref.g1_to_bytes(s),
                            128, 1)
        want = ref.g1_add(want, s)
        assert cp.xyzz_to_affine(acc) == want, f"{where} run step {i}"
        seen_inf += want is None
    assert seen_inf == 2 and seen_zz == 1 and want == p


# ------------------------------------------------- Jacobian forms, by bytes
def _dbl_2009_l(X, Y, Z):
    A, B = X * X % P, Y * Y % P
    C = B * B % P
    D = 2 * ((X + B) ** 2 - A - C) % P
    E = 3 * A % P
    X3 = (E * E - 2 * D) % P
    return X3, (E * (D - X3) - 8 * C) % P, 2 * Y * Z % P


def _add_2007_bl(X1, Y1, Z1, X2, Y2, Z2, mixed):
    """add-2007-bl, or madd-2007-bl (mixed, Z2 == 1 where the addend is a
    point), with the library's handling of the degenerate cases: an identity
    addend leaves the accumulator's bytes alone, an identity accumulator takes
    the addend's, and None is the identity the code sets itself."""
    if Z2 == 0:
        return X1, Y1, Z1
    if Z1 == 0:
        return X2, Y2, Z2
    U1, U2 = X1 * Z2 * Z2 % P, X2 * Z1 * Z1 % P
    S1, S2 = Y1 * pow(Z2, 3, P) % P, Y2 * pow(Z1, 3, P) % P
    H, r = (U2 - U1) % P, 2 * (S2 - S1) % P
    if H == 0:
        return _dbl_2009_l(X1, Y1, Z1) if r == 0 else None
    I = 4 * H * H % P
    J, V = H * I % P, U1 * I % P
    X3 = (r * r - J - 2 * V) % P
    Z3 = 2 * Z1 * H % P if mixed else 2 * Z1 * Z2 * H % P
    return X3, (r * (V - X3) - 2 * S1 * J) % P, Z3


def _jac_vals(pt, lam):
    if pt is None:
        return lam * lam % P, pow(lam, 3, P), 0
    return lam * lam * pt[0] % P, pow(lam, 3, P) * pt[1] % P, lam


def _jac_img(v):
    return eo.imgs_bytes([ONE, ONE, 0] if v is None
                         else [eo.fq_img(c) for c in v])


def check_jacobian_bytes(where):
    cs = eo.curve_cases()
    n = len(cs)
    left = b"".join(eo.jac_bytes(p, lam) for p, lam, _, _, _ in cs)
    aff = b"".join(ref.g1_to_bytes(q) for _, _, q, _, _ in cs)
    right = b"".join(eo.jac_bytes(q, lq) for _, _, q, lq, _ in cs)
    want_m = b"".join(
        _jac_img(_add_2007_bl(*_jac_vals(p, lam), *_jac_vals(q, 1), True))
        for p, lam, q, _, _ in cs)
    want_a = b"".join(
        _jac_img(_add_2007_bl(*_jac_vals(p, lam), *_jac_vals(q, lq), False))
        for p, lam, q, lq, _ in cs)
    assert cp.field_call(where, "g1_madd", "Fq", left, aff, 96, n) == want_m
    assert cp.field_call(where, "g1_add", "Fq", left, right, 96, n) == want_a
    ds = eo.dbl_cases()
    dl = b"".join(eo.jac_bytes(p, lam) for p, lam, _ in ds)
    want_d = b"".join(
        eo.jac_bytes(None, lam) if p is None
        else _jac_img(_dbl_2009_l(*_jac_vals(p, lam))) for p, lam, _ in ds)
    assert cp.field_call(where, "g1_dbl", "Fq", dl, None, 96, len(ds)) == want_d


# ------------------------------------------------------------ host (no GPU)
@pytest.mark.parametrize("op", XYZZ_OPS)
def test_host_xyzz(op):
    check_xyzz("host", op)


def test_host_xyzz_run():
    check_run("host")


def test_host_jacobian_bytes():
    check_jacobian_bytes("host")


# ------------------------------------------------------------------- device
@pytest.mark.gpu
@pytest.mark.parametrize("op", XYZZ_OPS)
def test_device_xyzz(op):
    assert check_xyzz("device", op) == check_xyzz("host", op), (
        f"{op}: device and host differ")


@pytest.mark.gpu
def test_device_xyzz_run():
    check_run("device")


@pytest.mark.gpu
def test_device_jacobian_bytes():
    check_jacobian_bytes("device")
