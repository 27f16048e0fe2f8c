"""ff_dot2, (a*b + c*d) * MONT^-1 mod m with one Montgomery reduction, on the
host and on the device at edge operands: bit-exact against Python integers and
against the bytes of ff_add(ff_mul(a, b), ff_mul(c, d)) from the field probe.

Operands are Montgomery images chosen directly (see edge_operands.py). The
catalogue is every ordered pair (a, b) of the specials below against a second
pair that walks the same list at another stride, then the cases named one by
one: all four m - 1 (the largest sum), a*b == -(c*d) (result 0), one pair
zero (the plain multiply), and seeded random quadruples. It runs in one batch
(no multiple of 64, so the last wave is partial and lanes sit on different
cases), as 65 elements and as one; the chain op applies ff_dot2 32 times from
every start with its output over one of its operands.
"""
import functools
import random

import pytest

import curve_probe_lib as cp
import edge_operands as eo

FIELD_NAMES = list(eo.FIELDS)
N_RANDOM = 300


@functools.lru_cache(maxsize=None)
def specials(m: int) -> tuple:
    xs = [0, 1, m - 1, m - 2, (m - 1) // 2, eo.ALL_ONES_LOW]
    xs += [1 << 32 * k for k in range(1, 8)]
    xs += [0xffffffff << 32 * k for k in range(7)] + [0x30644e72 << 224]
    assert all(0 <= x < m for x in xs) and len(set(xs)) == len(xs)
    return tuple(xs)


@functools.lru_cache(maxsize=None)
def quads(field: str) -> tuple:
    m = eo.FIELDS[field]
    sp = specials(m)
    ps = [(a, b) for a in sp for b in sp]
    out = [ab + ps[(5 * i + 3) % len(ps)] for i, ab in enumerate(ps)]
    out.append((m - 1,) * 4)
    out += [(a, b, m - a if a else 0, b) for a, b in ps]       # sum == 0 mod m
    out += [(a, b, 0, ps[(i + 1) % len(ps)][1]) for i, (a, b) in enumerate(ps)]
    out += [(0, ps[(i + 1) % len(ps)][0], a, b) for i, (a, b) in enumerate(ps)]
    rng = random.Random(0xd072 + m % 65537)
    out += [tuple(rng.randrange(m) for _ in range(4)) for _ in range(N_RANDOM)]
    return tuple(out)


def expect_dot2(m, a, b, c, d):
    return (a * b + c * d) * pow(eo.MONT, -1, m) % m


def expect_chain(m, a, b, c, d):
    x = a
    for _ in range(eo.CHAIN_STEPS // 2):
        x = expect_dot2(m, x, b, c, d)
        x = expect_dot2(m, a, x, x, d)
    return x


@functools.lru_cache(maxsize=None)
def expected(op: str, field: str) -> tuple:
    f = expect_dot2 if op == "dot2" else expect_chain
    return tuple(f(eo.FIELDS[field], *q) for q in quads(field))


def run(where, op, field, qs):
    a = eo.imgs_bytes(v for q in qs for v in q[:2])
    b = eo.imgs_bytes(v for q in qs for v in q[2:])
    return eo.imgs_from(cp.curve_call(where, op, field, a, b, 32, len(qs)))


def check(where, op, field, qs, want):
    got = run(where, op, field, qs)
    assert len(got) == len(want) == len(qs)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            pytest.fail(
                f"{where} {field} {op}: element {i} of {len(qs)}\n" +
                "".join(f"  {n}    = {eo.hx(v)}\n" for n, v in zip("abcd", qs[i])) +
                f"  got  = {eo.hx(g)}\n  want = {eo.hx(w)}")
    return got


def check_catalogue(where, op, field):
    qs, want = quads(field), expected(op, field)
    got = check(where, op, field, qs, want)
    m = eo.FIELDS[field]
    f = expect_dot2 if op == "dot2" else expect_chain
    spread65 = qs[7::len(qs) // 65][:65]
    assert len(spread65) == 65
    for sub in (spread65, ((m - 1,) * 4,)):
        check(where, op, field, sub, [f(m, *q) for q in sub])
    return got


def check_against_add_mul_mul(where, field):
    """The same bytes as the three-call form, computed by the field probe."""
    qs = quads(field)
    n = len(qs)
    col = [eo.imgs_bytes(q[k] for q in qs) for k in range(4)]
    ab = cp.field_call(where, "mul", field, col[0], col[1], 32, n)
    cd = cp.field_call(where, "mul", field, col[2], col[3], 32, n)
    ref = cp.field_call(where, "add", field, ab, cd, 32, n)
    assert eo.imgs_bytes(run(where, "dot2", field, qs)) == ref


def test_catalogue_is_what_the_tests_assume():
    for field, m in eo.FIELDS.items():
        qs = quads(field)
        assert 2000 < len(qs) < 3000 and len(qs) % 64 != 0
        assert all(0 <= v < m for q in qs for v in q)
        assert (m - 1,) * 4 in qs
        assert sum(1 for a, b, c, d in qs if (a * b + c * d) % m == 0) > 400
        assert any(c == 0 and a and b for a, b, c, d in qs)
        assert any(a == 0 and c and d for a, b, c, d in qs)
        # the largest sum stays inside the bound one trial subtract covers
        assert (2 * (m - 1) ** 2 + (eo.MONT - 1) * m) // eo.MONT < 2 * m


@pytest.mark.parametrize("field", FIELD_NAMES)
@pytest.mark.parametrize("op", ["dot2", "dot2chain"])
def test_host_dot2(op, field):
    check_catalogue("host", op, field)


@pytest.mark.parametrize("field", FIELD_NAMES)
def test_host_dot2_is_add_mul_mul(field):
    check_against_add_mul_mul("host", field)


def test_unserved_requests_are_refused():
    a = eo.img_bytes(1) * 2
    for where in ("host", "device"):  # refused before any HIP call
        for op, field in ((2, "Fq"), (20, "Fq"), ("x_dbl", "Fr")):
            rc, out = cp.curve_call_rc(where, op, field, a * 2, a * 2, 128, 1)
            assert rc == -1 and out == cp.FILL * 128, (where, op, field)


@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELD_NAMES)
@pytest.mark.parametrize("op", ["dot2", "dot2chain"])
def test_device_dot2(op, field):
    """Fq and Fr take the two-pair column form, FrCios the compiled CIOS."""
    dev = check_catalogue("device", op, field)
    assert dev == run("host", op, field, quads(field))


@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_device_dot2_is_add_mul_mul(field):
    check_against_add_mul_mul("device", field)
