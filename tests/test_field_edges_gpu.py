"""The edge operands of tests/edge_operands.py through the product's own
kernels, by the ABI of spectre_amd/ffi.py alone.

tests/test_field_probe.py shows ff.hpp and g1.hpp right in one code context;
these tests show the same operands right inside the kernels that ship:
k_fr_vec_op and k_fr_gate_eval (FrCios), the poly.hip kernels (the asm Fr
multiply) and the MSM (the asm Fq multiply and g1.hpp). Everything is
bit-exact against Python bigints on Montgomery images; the MSM also against
the C oracle."""
import random

import pytest

import edge_operands as eo

pytestmark = pytest.mark.gpu

R = eo.R
SP = eo.specials(R)                       # Fr special images
ONE = eo.MONT % R                         # image of 1
MINUS_ONE = R - ONE                       # image of -1
MINV = pow(eo.MONT, -1, R)
PAIRS = [(a, b) for a in SP for b in SP]  # every ordered pair
ZERO = bytes(32)
FILL = b"\xa5" * 32


def mul(a: int, b: int) -> int:
    return eo.expect("mul", R, a, b)


def first_diff(got: bytes, want, what: str, operands=None):
    """Assert that got is the images in want; name the first that is not."""
    gi = eo.imgs_from(got)
    assert len(gi) == len(want), what
    for i, (g, w) in enumerate(zip(gi, want)):
        if g != w:
            ops = ""
            if operands is not None:
                ops = "".join(f"\n  operand {eo.hx(x)}" for x in operands[i])
            pytest.fail(f"{what}: element {i}{ops}\n  got  {eo.hx(g)}\n"
                        f"  want {eo.hx(w)}")


class Dev:
    """Device buffers of one test, freed together."""

    def __init__(self, g):
        self.g, self.ptrs = g, []

    def put(self, data: bytes) -> int:
        p = self.g.malloc(max(len(data), 32))
        self.ptrs.append(p)
        if data:
            self.g.upload(p, data)
        return p

    def get(self, p: int, n: int) -> bytes:
        return self.g.download(p, 32 * n)

    def free(self):
        for p in self.ptrs:
            self.g.free(p)
        self.ptrs = []


@pytest.fixture
def dev(gpu):
    d = Dev(gpu)
    yield d
    d.free()


# ------------------------------------------------------------------ fr_vec_op
def test_vec_op_special_pairs(gpu, dev):
    n = len(PAIRS)
    a_b = eo.imgs_bytes(a for a, _ in PAIRS)
    b_b = eo.imgs_bytes(b for _, b in PAIRS)
    d_a, d_b, d_o = dev.put(a_b), dev.put(b_b), dev.put(FILL * n)
    for op, name in ((gpu.VEC_ADD, "add"), (gpu.VEC_SUB, "sub"),
                     (gpu.VEC_MUL, "mul")):
        gpu.fr_vec_op(op, d_a, d_b, None, d_o, n)
        first_diff(dev.get(d_o, n), [eo.expect(name, R, a, b) for a, b in PAIRS],
                   f"fr_vec_op {name}", PAIRS)
    for c in (0, ONE, R - 1, eo.ALL_ONES_LOW):
        cb = eo.img_bytes(c)
        gpu.fr_vec_op(gpu.VEC_SCALE, d_a, None, cb, d_o, n)
        first_diff(dev.get(d_o, n), [mul(a, c) for a, _ in PAIRS],
                   f"fr_vec_op scale by {eo.hx(c)}", PAIRS)
        gpu.fr_vec_op(gpu.VEC_ADD_SCALED, d_a, d_b, cb, d_o, n)
        first_diff(dev.get(d_o, n), [(a + mul(b, c)) % R for a, b in PAIRS],
                   f"fr_vec_op add_scaled by {eo.hx(c)}", PAIRS)
    assert dev.get(d_a, n) == a_b and dev.get(d_b, n) == b_b
    gpu.fr_vec_op(gpu.VEC_MUL, d_a, d_b, None, d_a, n)  # in place
    first_diff(dev.get(d_a, n), [mul(a, b) for a, b in PAIRS],
               "fr_vec_op mul in place", PAIRS)


# ------------------------------------------------------------------ gate_eval
def test_gate_eval_special_operands(gpu, dev):
    """gate_eval takes a power of two for n: the columns are padded with
    zeros up to the next one (64 for the specials, 4096 for the pairs)."""
    G = gpu
    n1 = 1 << (len(SP) - 1).bit_length()
    col = list(SP) + [0] * (n1 - len(SP))
    d_c = dev.put(eo.imgs_bytes(col))
    d_o = dev.put(FILL * n1)
    G.gate_eval([d_c], b"", [(G.GATE_COL, 0, 0), (G.GATE_NEG, 0, 0)], n1,
                d_out=d_o)
    first_diff(dev.get(d_o, n1), [(-a) % R for a in col], "gate_eval neg",
               [(a,) for a in col])
    n2 = 1 << (len(PAIRS) - 1).bit_length()
    pairs = PAIRS + [(0, 0)] * (n2 - len(PAIRS))
    d_a = dev.put(eo.imgs_bytes(a for a, _ in pairs))
    d_b = dev.put(eo.imgs_bytes(b for _, b in pairs))
    d_o2 = dev.put(FILL * n2)
    for op, name in ((G.GATE_MUL, "mul"), (G.GATE_SUB, "sub"),
                     (G.GATE_ADD, "add")):
        G.gate_eval([d_a, d_b], b"",
                    [(G.GATE_COL, 0, 0), (G.GATE_COL, 1, 0), (op, 0, 0)], n2,
                    d_out=d_o2)
        first_diff(dev.get(d_o2, n2),
                   [eo.expect(name, R, a, b) for a, b in pairs],
                   f"gate_eval {name}", pairs)


# --------------------------------------------------------------- fr_poly_eval
def test_poly_eval_two_coefficients(gpu, dev):
    """n = 2: [0, a] at z is a z, one asm Fr multiply in k_poly_tile_eval;
    [a, b] at the image of 1 is a + b and at the image of -1 is a - b."""
    k = len(SP)
    d_0a = dev.put(b"".join(ZERO + eo.img_bytes(a) for a in SP))
    for i, a in enumerate(SP):
        for j in range(0, k, 8):
            zs = SP[j:j + 8]
            got = gpu.fr_poly_eval(d_0a + 64 * i, 2,
                                   [eo.img_bytes(z) for z in zs])
            first_diff(b"".join(got), [mul(a, z) for z in zs],
                       "poly_eval [0, a] at z", [(a, z) for z in zs])
    d_ab = dev.put(b"".join(eo.img_bytes(a) + eo.img_bytes(b)
                            for a, b in PAIRS))
    pts = [eo.img_bytes(ONE), eo.img_bytes(MINUS_ONE)]
    for i, (a, b) in enumerate(PAIRS):
        got = gpu.fr_poly_eval(d_ab + 64 * i, 2, pts)
        first_diff(b"".join(got), [(a + b) % R, (a - b) % R],
                   "poly_eval [a, b] at 1 and at -1", [(a, b), (a, b)])


# --------------------------------------------------------- fr_poly_div_linear
def quotient(a, z):
    """q[n-1] = 0, q[i] = a[i+1] + z q[i+1], rem = a[0] + z q[0], on images."""
    q = [0] * len(a)
    for i in range(len(a) - 2, -1, -1):
        q[i] = (a[i + 1] + mul(z, q[i + 1])) % R
    return q, (a[0] + mul(z, q[0])) % R


@pytest.mark.parametrize("n", [2, 3])
def test_poly_div_linear_short(gpu, dev, n):
    """Every ordered pair (top coefficient, z) of specials; the lower
    coefficients are the specials that follow the top one."""
    k = len(SP)
    polys = [[SP[(i + n - 1 - t) % k] for t in range(n)] for i in range(k)]
    for p, i in zip(polys, range(k)):
        assert p[n - 1] == SP[i]
    d_a = dev.put(eo.imgs_bytes(x for p in polys for x in p))
    d_q = dev.put(FILL * (n * k * k))
    want_q, got_rem, want_rem, operands = [], [], [], []
    for j, z in enumerate(SP):
        for i, p in enumerate(polys):
            rem = gpu.fr_poly_div_linear(d_a + 32 * n * i, eo.img_bytes(z),
                                         d_q + 32 * n * (j * k + i), n)
            q, r = quotient(p, z)
            want_q += q
            got_rem.append(rem)
            want_rem.append(r)
            operands.append(tuple(p) + (z,))
    first_diff(b"".join(got_rem), want_rem, f"div n={n} remainder", operands)
    first_diff(dev.get(d_q, n * k * k), want_q, f"div n={n} quotient",
               [o for o in operands for _ in range(n)])


# ------------------------------------------------------------ fr_batch_invert
@pytest.mark.parametrize("order", ["catalogue", "reversed"])
def test_batch_invert_specials(gpu, dev, order):
    xs = list(SP) if order == "catalogue" else list(reversed(SP))
    want = [eo.expect("inv", R, x, 0) for x in xs]
    # zero stays zero; 1 and -1 are their own inverses, on images too
    for x, w in zip(xs, want):
        if x in (0, ONE, MINUS_ONE):
            assert w == x
    n = len(xs)
    d_in, d_out = dev.put(eo.imgs_bytes(xs)), dev.put(FILL * (n + 1))
    gpu.fr_batch_invert(d_in, d_out, n)
    assert dev.get(d_out, n + 1)[32 * n:] == FILL
    first_diff(dev.get(d_out, n), want, f"batch_invert {order}",
               [(x,) for x in xs])
    gpu.fr_batch_invert(d_in, d_in, n)
    first_diff(dev.get(d_in, n), want, f"batch_invert {order} in place",
               [(x,) for x in xs])


# ----------------------------------------------------------- fr_grand_product
def test_grand_product_specials(gpu, dev):
    def prefixes(xs):
        out, acc = [ONE], ONE
        for x in xs:
            acc = mul(acc, x)
            out.append(acc)
        return out

    nz = [x for x in SP if x]
    planted = nz[:len(nz) // 2] + [0] + nz[len(nz) // 2:]
    for xs, what in ((nz, "nonzero specials"), (planted, "zero planted")):
        n = len(xs)
        want = prefixes(xs)
        d_num, d_z = dev.put(eo.imgs_bytes(xs)), dev.put(FILL * (n + 1))
        last = gpu.fr_grand_product(d_num, None, None, d_z, n)
        assert dev.get(d_z, n + 1)[32 * n:] == FILL
        first_diff(dev.get(d_z, n) + last, want, f"grand_product {what}")
    assert all(w == 0 for w in want[len(nz) // 2 + 1:]) and want[len(nz) // 2]


# ------------------------------------------------------------------------ msm
PTS = [p for p in eo.edge_points() if p is not None]
RND = random.Random(0xed9e)
RAND_SCALAR = RND.randrange(R)
# every 16-bit window but the top one (a scalar < r has a top window below
# 0x3065) is above 2^15 and below 0xffff: each of those digits is negative
NEG_DIGIT_SCALARS = [
    int("8001" * 15, 16), int("fffe" * 15, 16),
    int("".join(f"{RND.randrange(0x8001, 0xffff):04x}" for _ in range(15)), 16),
    (0x3063 << 240) | int("c000" * 15, 16),
]
assert all(s < R for s in NEG_DIGIT_SCALARS)


def msm_case_a():
    return [(s, p) for p in PTS for s in (1, 2, R - 1, (1 << 16) - 1)]


def msm_case_b():
    scal = [1, R - 1, (1 << 16) - 1, RAND_SCALAR, 1 << 15, (1 << 15) + 1]
    out = []
    for p, s in zip(PTS, scal):
        out += [(s, p), (s, eo.ref.g1_neg(p))]
    return out


def msm_case_c():
    scal = [1, 2, R - 1, (1 << 16) - 1, RAND_SCALAR, NEG_DIGIT_SCALARS[0]]
    return [(s, p) for p, s in zip(PTS, scal) for _ in range(9)]


def msm_case_d():
    out = []
    for i, s in enumerate(NEG_DIGIT_SCALARS):
        out += [(s, None), (s, PTS[i % len(PTS)])]
    return out


def check_msm(g, oracle, terms, what: str, want="bigint"):
    n = len(terms)
    assert n < 100
    bases = b"".join(eo.ref.g1_to_bytes(p) for _, p in terms)
    scalars = b"".join(eo.ref.to_canon_bytes(s) for s, _ in terms)
    if want == "bigint":
        want = eo.ref.g1_to_bytes(eo.ref.msm([s for s, _ in terms],
                                             [p for _, p in terms]))
    got = g.msm(bases, scalars, n, canonical=True)
    assert got == want, (
        f"msm {what}: got {got.hex()} want {want.hex()}\n" + "\n".join(
            f"  {s:#x} * {eo.desc_point(p)}" for s, p in terms[:12]))
    assert oracle.msm(bases, scalars, n, scalars_canonical=True) == want, \
        f"oracle differs from bigints at {what}"


def test_msm_each_edge_point(gpu, oracle):
    for s, p in msm_case_a():
        check_msm(gpu, oracle, [(s, p)], "single term")
    check_msm(gpu, oracle, msm_case_a(), "all single terms together")


def test_msm_point_and_negation_cancel(gpu, oracle):
    terms = msm_case_b()
    for i in range(0, len(terms), 2):
        check_msm(gpu, oracle, terms[i:i + 2], "P and -P", want=bytes(64))
    check_msm(gpu, oracle, terms, "all P and -P together", want=bytes(64))


def test_msm_repeated_point_doubles_in_one_run(gpu, oracle):
    terms = msm_case_c()
    for i in range(0, len(terms), 9):
        check_msm(gpu, oracle, terms[i:i + 9], "one point nine times")
    check_msm(gpu, oracle, terms, "every point nine times")


def test_msm_identity_base_with_negative_digits(gpu, oracle):
    """k_bucket_acc negates the base's y before g1j_madd_ip tests it for
    the identity: ff_neg(0) has to be 0."""
    for s in NEG_DIGIT_SCALARS:
        check_msm(gpu, oracle, [(s, None)], "identity alone", want=bytes(64))
    only_inf = [(s, None) for s in NEG_DIGIT_SCALARS]
    check_msm(gpu, oracle, only_inf, "identities only", want=bytes(64))
    check_msm(gpu, oracle, msm_case_d(), "identities among points")


def test_msm_all_edges_shuffled(oracle):
    from spectre_amd import SpectreGpu
    terms = msm_case_a() + msm_case_b() + msm_case_c() + msm_case_d()
    random.Random(0x5af1e).shuffle(terms)
    g = SpectreGpu([0])
    try:
        for e in (4, 0):
            g.set_msm_acc_entries(e)
            check_msm(g, oracle, terms, f"shuffled, acc entries {e}")
    finally:
        g.set_msm_acc_entries(0)
        g.close()
