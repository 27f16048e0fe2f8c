"""Edge operands for the field and curve layer, and their bigint expectations.

TEST INFRASTRUCTURE, shared by test_field_probe.py and
test_field_edges_gpu.py. A kernel sees the Montgomery *image* of a field
element, the eight 32-bit limbs in memory, so the catalogue chooses images
directly, as integers x with 0 <= x < m, and the reference below is written on
images (MONT = 2^256; bn254_ref calls it MONT because R is its Fr modulus):

    mul              a b MONT^-1 mod m
    add / sub / neg  the plain modular op
    inv              MONT^2 a^-1 mod m, and 0 for a = 0
    from_mont        a MONT^-1 mod m
    to_mont          a MONT mod m
    pow_u32          MONT (a MONT^-1)^e mod m

1 and m - 1 are their own inverses as canonical values; their images are
MONT mod m and m - (MONT mod m), and `inv` maps each of those to itself.
Everything is computed once per process and must be left unchanged by its
users.
"""
import functools
import importlib.util
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "bn254_ref", os.path.join(HERE, "golden", "bn254_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)

P, R, MONT = ref.P, ref.R, ref.MONT
# field name -> modulus; the probe's field codes are the positions in this dict
FIELDS = {"Fq": P, "Fr": R, "FrCios": R}
N_RANDOM_PAIRS = 500
CHAIN_STEPS = 32
# top limb one below the moduli's (both 0x30644e72), every lower limb all
# ones: the reduced operand with the largest column sums
ALL_ONES_LOW = (0x30644e71 << 224) | ((1 << 224) - 1)
assert ALL_ONES_LOW < R < P


def img_bytes(x: int) -> bytes:
    return x.to_bytes(32, "little")


def imgs_bytes(xs) -> bytes:
    return b"".join(x.to_bytes(32, "little") for x in xs)


def imgs_from(data: bytes) -> list[int]:
    return [int.from_bytes(data[i:i + 32], "little")
            for i in range(0, len(data), 32)]


def hx(x: int) -> str:
    return f"0x{x:064x}"


# ------------------------------------------------------------------ specials
@functools.lru_cache(maxsize=None)
def specials(m: int) -> tuple:
    """The special images of the field with modulus m: in order, without
    repeats, the ones >= m dropped."""
    one = MONT % m
    low128 = (1 << 128) - 1
    xs = [0, 1, 2, 3, m - 1, m - 2, m - 3, (m - 1) // 2, (m + 1) // 2,
          one, m - one, MONT * MONT % m, ALL_ONES_LOW]
    for k in range(1, 8):
        xs += [1 << 32 * k, (1 << 32 * k) - 1, (1 << 32 * k) + 1,
               m - (1 << 32 * k), 0xffffffff << 32 * (k - 1)]
    xs += [int("00000000ffffffff" * 4, 16) % m,
           int("ffffffff00000000" * 4, 16) % m,
           m & ~low128, m & low128, 1 << 253, (1 << 253) - 1]
    out = []
    for x in xs:
        if 0 <= x < m and x not in out:
            out.append(x)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def golden_cases(field: str) -> tuple:
    """The committed fixture cases as (a, b, {op: image}) on images."""
    name = "fq_arith.json" if field == "Fq" else "fr_arith.json"
    with open(os.path.join(HERE, "golden", name)) as f:
        fix = json.load(f)
    assert int(fix["modulus"], 16) == FIELDS[field]

    def img(h):
        return int.from_bytes(bytes.fromhex(h), "little")

    return tuple(
        (img(c["a_mont"]), img(c["b_mont"]),
         {op: img(c[op]) for op in ("add", "sub", "mul", "sqr", "inv")})
        for c in fix["cases"])


@functools.lru_cache(maxsize=None)
def pairs(field: str) -> tuple:
    """Every ordered pair of specials, N_RANDOM_PAIRS seeded random pairs,
    then the fixture pairs (so golden_cases(field)[j] is pairs(field)[-len + j])."""
    m = FIELDS[field]
    sp = specials(m)
    out = [(a, b) for a in sp for b in sp]
    rng = random.Random(0x5eed0000 + m % 65537)
    out += [(rng.randrange(m), rng.randrange(m))
            for _ in range(N_RANDOM_PAIRS)]
    out += [(a, b) for a, b, _ in golden_cases(field)]
    return tuple(out)


def corner_pair(field: str):
    """The one-element batch: both operands the all-ones-low image."""
    return ((ALL_ONES_LOW, ALL_ONES_LOW),)


def spread65(field: str) -> tuple:
    """65 pairs spread over the whole list (one full wave and one lane)."""
    ps = pairs(field)
    step = len(ps) // 65
    return ps[7::step][:65]


# ------------------------------------------------------------ field reference
def expect(op: str, m: int, a: int, b: int) -> int:
    minv = pow(MONT, -1, m)
    if op in ("mul", "mul_cios"):
        return a * b * minv % m
    if op == "sqr":
        return a * a * minv % m
    if op == "add":
        return (a + b) % m
    if op == "sub":
        return (a - b) % m
    if op == "neg":
        return (-a) % m
    if op == "inv":
        return MONT * MONT * pow(a, -1, m) % m if a else 0
    if op == "to_mont":
        return a * MONT % m
    if op == "from_mont":
        return a * minv % m
    if op == "pow_u32":
        return MONT * pow(a * minv, b & 0xffffffff, m) % m
    if op == "mulchain":
        x = a
        for i in range(CHAIN_STEPS):
            x = x * (a if i & 1 else b) * minv % m
        return x
    if op == "sqrchain":
        x = a
        for _ in range(CHAIN_STEPS):
            x = x * x * minv % m
        return x
    raise ValueError(op)


@functools.lru_cache(maxsize=None)
def expected(op: str, field: str) -> tuple:
    """expect(op) over pairs(field), computed once."""
    m = FIELDS[field]
    return tuple(expect(op, m, a, b) for a, b in pairs(field))


# ------------------------------------------------------------ curve catalogue
def _sqrt_q(v: int):
    y = pow(v, (P + 1) // 4, P)
    return y if y * y % P == v % P else None


def _point_with_x(x: int):
    y = _sqrt_q((x * x * x + 3) % P)
    return None if y is None else (x, y)


@functools.lru_cache(maxsize=None)
def edge_points() -> tuple:
    """Affine points (canonical coordinates), the identity (None) last: x = 1,
    2, 2^64 - 1 and q - 1, and the two points whose x *image* is the largest
    value <= ALL_ONES_LOW that lies on the curve."""
    pts = []
    for x in (1, 2, (1 << 64) - 1, P - 1):
        pt = _point_with_x(x)
        assert pt is not None, f"x = {x} is not on the curve"
        pts.append(pt)
    assert _point_with_x(0) is None and _point_with_x((1 << 32) - 1) is None
    minv = pow(MONT, -1, P)
    ximg = ALL_ONES_LOW
    while _point_with_x(ximg * minv % P) is None:
        ximg -= 1
    pt = _point_with_x(ximg * minv % P)
    pts += [pt, ref.g1_neg(pt)]
    assert all(ref.g1_is_on_curve(p) for p in pts)
    return tuple(pts) + (None,)


@functools.lru_cache(maxsize=None)
def lambdas() -> tuple:
    """Canonical Z values a Jacobian operand is presented with."""
    return (1, 2, P - 1, random.Random(0x1a3bda).randrange(3, P - 1))


def fq_img(v: int) -> int:
    return v * MONT % P


def jac_bytes(pt, lam: int) -> bytes:
    """(lam^2 x, lam^3 y, lam) as a 96-byte Jacobian image; the identity is
    (lam^2, lam^3, 0)."""
    x, y = pt if pt is not None else (1, 1)
    z = lam if pt is not None else 0
    return imgs_bytes([fq_img(lam * lam * x % P), fq_img(pow(lam, 3, P) * y % P),
                       fq_img(z)])


def jac_to_affine(data: bytes):
    """A 96-byte Jacobian image -> affine canonical (x, y), None iff Z = 0.
    Every coordinate must be a reduced image."""
    X, Y, Z = imgs_from(data)
    assert X < P and Y < P and Z < P, "unreduced Jacobian coordinate"
    if Z == 0:
        return None
    minv = pow(MONT, -1, P)
    X, Y, Z = X * minv % P, Y * minv % P, Z * minv % P
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * pow(zi, 3, P) % P)


def desc_point(pt) -> str:
    return "inf" if pt is None else f"({hx(fq_img(pt[0]))}, {hx(fq_img(pt[1]))})"


@functools.lru_cache(maxsize=None)
def curve_cases() -> tuple:
    """(P, lam, Q, lam_q, P + Q) for every ordered pair of edge points, Q as
    is and negated, P under each lambda; lam_q is the Z that Q takes where an
    op wants it in Jacobian form (the next lambda round, so both sides have
    Z != 1 somewhere). With Z != 1 on the left this covers generic addition,
    P + P, P + (-P) and the identity on either side and on both."""
    pts, lams = edge_points(), lambdas()
    out = []
    for p in pts:
        for q in pts:
            for qq in (q, ref.g1_neg(q)):
                for i, lam in enumerate(lams):
                    out.append((p, lam, qq, lams[(i + 1) % len(lams)],
                                ref.g1_add(p, qq)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def dbl_cases() -> tuple:
    """(P, lam, 2P) over the same points and lambdas."""
    return tuple((p, lam, ref.g1_add(p, p))
                 for p in edge_points() for lam in lambdas())
