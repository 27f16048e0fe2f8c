"""CPU checks that pin tests/multiopen_ref.py itself, in integers only: the
chained quotient and its remainders against the Newton reconstruction and a
schoolbook division by the expanded Z_S, for random, 0, 1 and repeated roots;
and the two-set opening identity that tests/test_multiopen_gpu.py closes on
the device."""
import importlib.util
import os
import random

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "multiopen_ref", os.path.join(HERE, "multiopen_ref.py"))
mr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mr)
R = mr.R


def root_sets(rng):
    z = [rng.randrange(R) for _ in range(8)]
    return [[z[0]], [0], [1], [z[0], z[1]], [0, 1, z[2]], [z[3], z[3]],
            [z[4], 0, z[4], 1, z[4]], [1, 1], [0, 0, 0], z,
            [R - 1, z[5], R - 1]]


@pytest.mark.parametrize("n", [1, 2, 3, 9, 40])
def test_chained_division_is_division_by_the_set(n):
    rng = random.Random(0x6d6f + n)
    a = [rng.randrange(R) for _ in range(n)]
    a[rng.randrange(n)] = 0
    for roots in root_sets(rng):
        q, rems = mr.div_roots(a, roots)
        assert len(q) == n and len(rems) == len(roots)
        top = min(len(roots), n)
        assert q[n - top:] == [0] * top
        # a == Z_S q + Newton(rems)
        z_s = mr.vanishing(roots)
        r = mr.newton(rems, roots)
        back = mr.poly_add(mr.poly_mul(z_s, mr.trim(q)), r)
        assert mr.trim(back) == mr.trim(a), roots
        # the Newton form agrees with a at every root
        for z in roots:
            assert mr.horner(r, z) == mr.horner(a, z)
        # and with a schoolbook division by the expanded Z_S
        sq, sr = mr.schoolbook_divmod(a, z_s)
        assert mr.trim(sq) == mr.trim(q)
        assert mr.trim(sr) == mr.trim(r)
        assert len(r) <= len(roots)


def test_first_remainder_is_the_evaluation():
    rng = random.Random(0x6d70)
    a = [rng.randrange(R) for _ in range(33)]
    z = [rng.randrange(R) for _ in range(3)]
    _, rems = mr.div_roots(a, z)
    assert rems[0] == mr.horner(a, z[0])
    q1, rem1 = mr.div_linear(a, z[0])
    assert rem1 == rems[0] and rems[1] == mr.horner(q1, z[1])


def test_exact_product_has_zero_remainders():
    rng = random.Random(0x6d71)
    roots = [rng.randrange(R), 0, 1, 1]
    q0 = [rng.randrange(R) for _ in range(20)]
    a = mr.poly_mul(mr.vanishing(roots), q0)
    q, rems = mr.div_roots(a, roots)
    assert rems == [0] * 4
    assert q == q0 + [0] * 4


def test_newton_from_evals_matches_the_remainders():
    rng = random.Random(0x6d72)
    a = [rng.randrange(R) for _ in range(50)]
    for k in (1, 2, 3, 8):
        roots = [rng.randrange(R) for _ in range(k)]
        _, rems = mr.div_roots(a, roots)
        evals = [mr.horner(a, z) for z in roots]
        assert mr.newton_from_evals(roots, evals) == rems


def test_lincomb_is_horner_in_y():
    rng = random.Random(0x6d73)
    n, m = 17, 5
    polys = [[rng.randrange(R) for _ in range(n)] for _ in range(m)]
    y = rng.randrange(R)
    # halo2: acc = acc * y + p, first polynomial first
    acc = [0] * n
    for p in polys:
        acc = [(s * y + c) % R for s, c in zip(acc, p)]
    coeffs = [pow(y, m - 1 - k, R) for k in range(m)]
    assert mr.lincomb(polys, coeffs, n) == acc
    assert mr.lincomb(polys, [0] * m, n) == [0] * n
    assert mr.lincomb(polys[:1], [1], n) == polys[0]


def test_two_set_opening_identity():
    """S_1 = {x} with three polynomials, S_2 = {x, wx, w^2 x} with two: L(u)
    is zero, so W = L / (X - u) is exact, and W's defining identity holds at
    a fresh point."""
    rng = random.Random(0x6d74)
    log_n = 6
    n = 1 << log_n
    w = mr.ref.fr_root_of_unity(log_n)
    x, y, v, u, s = (rng.randrange(R) for _ in range(5))
    p1 = [[rng.randrange(R) for _ in range(n)] for _ in range(3)]
    p2 = [[rng.randrange(R) for _ in range(n)] for _ in range(2)]
    s1, s2 = [x], [x, w * x % R, w * w * x % R]
    o = mr.shplonk_open([(s1, p1), (s2, p2)], y, v, u, n)
    assert o["W_rem"] == 0
    assert o["W"][n - 1] == 0
    assert o["z_t"] == mr.horner(mr.vanishing(s2), u)
    assert o["zdiff"] == [mr.horner(mr.vanishing(s2[1:]), u), 1]
    # the remainders are the interpolants of the combined evaluations
    for (pts, polys), rems, f in zip([(s1, p1), (s2, p2)], o["rems"], o["f"]):
        evals = [sum(pow(y, k, R) * mr.horner(p, z)
                     for k, p in enumerate(polys)) % R for z in pts]
        assert mr.newton_from_evals(pts, evals) == rems
        assert evals == [mr.horner(f, z) for z in pts]
    # (s - u) W(s) == L(s), and L(s) from its definition
    l_s = sum(pow(v, i, R) * o["zdiff"][i] *
              (mr.horner(o["f"][i], s) - o["r_u"][i]) for i in range(2))
    l_s = (l_s - o["z_t"] * mr.horner(o["h"], s)) % R
    assert mr.horner(o["L"], s) == l_s
    assert (s - u) * mr.horner(o["W"], s) % R == l_s
    # a wrong evaluation opens it
    bad = list(o["L"])
    bad[0] = (bad[0] + 1) % R
    assert mr.div_linear(bad, u)[1] != 0
