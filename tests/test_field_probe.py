"""ff.hpp and g1.hpp called directly, on the host and on the device, at the edge
operands of tests/edge_operands.py, bit-exact against Python bigints.

The probe library (tests/probe/field_probe.hip, built by build() into
spectre_amd/libspectre_ffprobe.so) has a host entry and a device entry of one
signature. The CPU tests send the whole catalogue through the host entry, so a
wrong header fails without a GPU; the `gpu` tests send it through the device
entry, where Fq and Fr multiply with the asm column form and FrCios with the
compiled CIOS. A whole catalogue goes in one launch (about 3300 elements, so
the last wave is partly filled), and again as batches of 1 and 65. A missing
library fails the test; nothing here skips."""
import ctypes
import os

import pytest

import edge_operands as eo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_LIB = os.path.join(REPO, "spectre_amd", "libspectre_ffprobe.so")

# op codes of tests/probe/field_probe.hip
OPS = {"mul": 0, "sqr": 1, "add": 2, "sub": 3, "neg": 4, "inv": 5,
       "to_mont": 6, "from_mont": 7, "pow_u32": 8, "mul_cios": 9,
       "mulchain": 10, "sqrchain": 11, "g1_dbl": 16, "g1_madd": 17,
       "g1_add": 18}
FIELD_CODE = {name: i for i, name in enumerate(eo.FIELDS)}
FIELD_OPS = ["mul", "sqr", "add", "sub", "neg", "inv", "to_mont", "from_mont",
             "pow_u32"]
CHAINS = ["mulchain", "sqrchain"]
FIELD_NAMES = list(eo.FIELDS)
ASM_FIELDS = ["Fq", "Fr"]
FILL = b"\x5a"

_lib = None


def probe():
    global _lib
    if _lib is None:
        if not os.path.exists(PROBE_LIB):
            pytest.fail(f"{PROBE_LIB} not found; run __graft_entry__.build()")
        lib = ctypes.CDLL(PROBE_LIB)
        for fn in (lib.ffprobe_host, lib.ffprobe_device):
            fn.restype = ctypes.c_int
            fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                           ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64]
        _lib = lib
    return _lib


def call_rc(where: str, op: str, field: str, a: bytes, b, out_elem: int,
            n: int):
    """(rc, output bytes); the output buffer has one element more than n,
    which has to stay untouched."""
    fn = probe().ffprobe_host if where == "host" else probe().ffprobe_device
    out = ctypes.create_string_buffer(FILL * (out_elem * (n + 1)),
                                      out_elem * (n + 1))
    rc = fn(OPS[op], FIELD_CODE[field], a, b, out, n)
    raw = out.raw
    assert raw[out_elem * n:] == FILL * out_elem, f"{op} wrote past n"
    return rc, raw[:out_elem * n]


def call(where, op, field, a, b, out_elem, n) -> bytes:
    rc, out = call_rc(where, op, field, a, b, out_elem, n)
    assert rc == 0, f"ffprobe_{where}({op}, {field}) returned {rc}"
    return out


def run_field(where: str, op: str, field: str, ps) -> list[int]:
    a = eo.imgs_bytes(p[0] for p in ps)
    b = eo.imgs_bytes(p[1] for p in ps)
    return eo.imgs_from(call(where, op, field, a, b, 32, len(ps)))


def check_field(where, op, field, ps, want, ref_op=None):
    got = run_field(where, op, field, ps)
    assert len(got) == len(want) == len(ps)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            pytest.fail(
                f"{where} {field} {op}: element {i} of {len(ps)}\n"
                f"  a    = {eo.hx(ps[i][0])}\n  b    = {eo.hx(ps[i][1])}\n"
                f"  got  = {eo.hx(g)}\n  want = {eo.hx(w)} ({ref_op or op})")
    return got


def check_catalogue(where: str, op: str, field: str):
    """The whole pair list in one batch, then batches of 65 and 1; and where
    the fixtures carry the op, their committed result as a second
    expectation."""
    ps, want = eo.pairs(field), eo.expected(op, field)
    got = check_field(where, op, field, ps, want)
    cases = eo.golden_cases(field)
    if op in cases[0][2]:
        tail = got[len(ps) - len(cases):]
        for (a, b, res), g in zip(cases, tail):
            assert g == res[op], (
                f"{where} {field} {op} differs from the committed fixture at "
                f"a = {eo.hx(a)}, b = {eo.hx(b)}")
    m = eo.FIELDS[field]
    for small in (eo.spread65(field), eo.corner_pair(field)):
        check_field(where, op, field, small,
                    [eo.expect(op, m, a, b) for a, b in small])


def curve_inputs(op: str):
    """(a bytes, b bytes or None, expected affine sums, descriptions) of a
    curve op; g1_add_swapped is g1_add with the operands exchanged, so the
    catalogue's left side becomes the addend."""
    if op == "g1_dbl":
        cs = eo.dbl_cases()
        return (b"".join(eo.jac_bytes(p, lam) for p, lam, _ in cs), None,
                [c[2] for c in cs],
                [f"dbl {eo.desc_point(p)} Z = {eo.hx(eo.fq_img(lam))}"
                 for p, lam, _ in cs])
    cs = eo.curve_cases()
    left = b"".join(eo.jac_bytes(p, lam) for p, lam, _, _, _ in cs)
    if op == "g1_madd":
        right = b"".join(eo.ref.g1_to_bytes(q) for _, _, q, _, _ in cs)
    else:
        right = b"".join(eo.jac_bytes(q, lq) for _, _, q, lq, _ in cs)
    if op == "g1_add_swapped":
        left, right = right, left
    return (left, right, [c[4] for c in cs],
            [f"{op} P = {eo.desc_point(p)} Z = {eo.hx(eo.fq_img(lam))}, "
             f"Q = {eo.desc_point(q)} Z = {eo.hx(eo.fq_img(lq))}"
             for p, lam, q, lq, _ in cs])


CURVE_OPS = ["g1_dbl", "g1_madd", "g1_add", "g1_add_swapped"]


def check_curve(where: str, op: str) -> bytes:
    a, b, want, desc = curve_inputs(op)
    n = len(want)
    out = call(where, op.replace("_swapped", ""), "Fq", a, b, 96, n)
    for i in range(n):
        got = eo.jac_to_affine(out[96 * i:96 * (i + 1)])
        assert got == want[i], (
            f"{where} case {i}: {desc[i]}\n  got  {eo.desc_point(got)}\n"
            f"  want {eo.desc_point(want[i])}")
    return out


# ---------------------------------------------------------------- catalogue
def test_catalogue_is_what_the_tests_assume():
    for field, m in eo.FIELDS.items():
        sp = eo.specials(m)
        assert len(sp) >= 53 and len(set(sp)) == len(sp)
        assert all(0 <= x < m for x in sp)
        for x in (0, 1, m - 1, eo.MONT % m, m - eo.MONT % m, eo.ALL_ONES_LOW):
            assert x in sp
        ps = eo.pairs(field)
        assert len(ps) >= len(sp) ** 2 + 500
        assert 3000 < len(ps) < 4000 and len(ps) % 64 != 0
        assert all(a < m and b < m for a, b in ps)
        assert len(eo.spread65(field)) == 65
        # a + b == m exactly, a == b, and zero all occur
        assert any(a + b == m for a, b in ps)
        assert any(a == b and a for a, b in ps) and (0, 0) in ps
        # the reference agrees with the committed fixtures
        for a, b, res in eo.golden_cases(field):
            for op, img in res.items():
                assert eo.expect(op, m, a, b) == img, (field, op)
        # what "self-inverse" means on images
        one = eo.MONT % m
        assert eo.expect("inv", m, one, 0) == one
        assert eo.expect("inv", m, m - one, 0) == m - one
        assert eo.expect("inv", m, 0, 0) == 0
    assert len(eo.edge_points()) == 7 and eo.edge_points()[-1] is None
    assert len(eo.curve_cases()) == 392 and len(eo.dbl_cases()) == 28
    kinds = {"generic": 0, "double": 0, "opposite": 0, "inf": 0}
    for p, _, q, _, s in eo.curve_cases():
        if p is None or q is None:
            kinds["inf"] += 1
        elif p == q:
            kinds["double"] += 1
        elif s is None:
            kinds["opposite"] += 1
        else:
            kinds["generic"] += 1
    assert all(kinds.values()), kinds


# ------------------------------------------------------- host path (no GPU)
@pytest.mark.parametrize("field", FIELD_NAMES)
@pytest.mark.parametrize("op", FIELD_OPS)
def test_host_field_op(op, field):
    check_catalogue("host", op, field)


@pytest.mark.parametrize("field", FIELD_NAMES)
@pytest.mark.parametrize("op", CHAINS)
def test_host_chain(op, field):
    check_catalogue("host", op, field)


@pytest.mark.parametrize("op", CURVE_OPS)
def test_host_curve(op):
    check_curve("host", op)


def test_unserved_requests_are_refused():
    """An op or field the probe does not serve returns -1 and writes
    nothing, on the host; the explicit CIOS op is a device op."""
    a = b = eo.img_bytes(1)
    lib = probe()
    for op, field in (("mul_cios", "Fq"), ("mul_cios", "FrCios"),
                      ("g1_dbl", "Fr")):
        rc, out = call_rc("host", op, field, a * 3, b * 3,
                          96 if op.startswith("g1") else 32, 1)
        assert rc == -1 and out == FILL * len(out), (op, field)
    out = ctypes.create_string_buffer(FILL * 32, 32)
    for fn in (lib.ffprobe_host, lib.ffprobe_device):  # refused before any HIP call
        assert fn(12, 0, a, b, out, 1) == -1
        assert fn(19, 0, a, b, out, 1) == -1
        assert fn(0, 3, a, b, out, 1) == -1
        assert fn(0, 0, None, b, out, 1) == -1
        assert fn(0, 0, a, None, out, 1) == -1
        assert fn(0, 0, a, b, out, (1 << 24) + 1) == -1
    assert out.raw == FILL * 32
    assert lib.ffprobe_host(0, 0, a, b, out, 0) == 0 and out.raw == FILL * 32


# ------------------------------------------------------------------- device
@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELD_NAMES)
@pytest.mark.parametrize("op", FIELD_OPS)
def test_device_field_op(op, field):
    check_catalogue("device", op, field)


@pytest.mark.gpu
@pytest.mark.parametrize("field", ASM_FIELDS)
def test_device_asm_mul_vs_cios_vs_bigint(field):
    """The asm column multiply, the compiled CIOS and bigints, three ways."""
    ps, want = eo.pairs(field), eo.expected("mul", field)
    cios = check_field("device", "mul_cios", field, ps, want)
    asm = check_field("device", "mul", field, ps, want)
    check_field("device", "mul", field, ps, cios, ref_op="device mul_cios")
    assert asm == cios == list(want)
    m = eo.FIELDS[field]
    for small in (eo.spread65(field), eo.corner_pair(field)):
        check_field("device", "mul_cios", field, small,
                    [eo.expect("mul", m, a, b) for a, b in small])
    # FrCios has no separate CIOS op: its ff_mul is the CIOS
    rc, _ = call_rc("device", "mul_cios", "FrCios", eo.img_bytes(1),
                    eo.img_bytes(1), 32, 1)
    assert rc == -1


@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELD_NAMES)
@pytest.mark.parametrize("op", CHAINS)
def test_device_chain(op, field):
    """32 multiplies back to back, unrolled in the kernel: the neighbourhood
    in which one asm block follows another."""
    check_catalogue("device", op, field)


@pytest.mark.gpu
@pytest.mark.parametrize("op", CURVE_OPS)
def test_device_curve(op):
    """Against the bigint affine sum, and byte for byte against the host
    build of the same formulas."""
    dev = check_curve("device", op)
    assert dev == check_curve("host", op), f"{op}: device and host differ"
