"""spectre_gpu_ntt_fr_device and spectre_gpu_ntt_fr_extend_device at 2^25 ..
2^28, the sizes ntt_split sends through three passes, against the split
reference of tests/ntt_split_ref.py: n = n1 * 2^23, so every leg is n1 = 4,
8, 16, 32 linear combinations (fr_lincomb) and forward coset NTTs at 2^23,
the (11,12) split that test_ntt_shapes_gpu compares with the oracle. Nothing
leaves the device but a verdict per slice, so the oracle's minutes at these
sizes are not needed. tests/test_ntt_split.py checks that SIZES and EXTEND
reach every pass class of the default rule at 25..28.

test_machinery_vs_oracle_at_2pow20 comes first: the same device backend at
2^20 (n1 = 4) next to oracle.ntt on the downloaded vector. It shows that the
pointers shared with torch, the strided compare and the coefficient tables
agree with the oracle here; what follows rests on it.

Per size: the forward, coset and inverse legs against the reference, the
inverse coset leg as icoset(coset(x)) == x (sound once the coset leg is
pinned: x is dense and random); eight outputs of the forward and coset legs
against fr_poly_eval at g * w^j, a path that shares nothing with the NTT
(poly.hip, asm multiply); ntt_extend_device against the coset leg of the
zero-padded buffer, all N elements.

Input: dense and not periodic, generated on the device with a fixed seed per
size: three low limbs over the int64 range, the top limb below r's top limb,
so every element is below r; 0 and r - 1 planted at index 0, n - 1 and in
each third of the vector.

The module owns its context: the call arena grows to 2^log_n elements (8 GiB
at 2^28) and is released when the module ends. Peak device memory is about
four vectors of the item's size (x, X, the arena, the pieces): 4 GiB at 2^25,
32 GiB at 2^28. An item at 27 or 28 skips only when the device shows less
free memory than that, and prints both numbers; 25 and 26 never skip.

Wall time per item on an MI355X, pytest --durations=0, the whole module
6.4 s with nothing skipped:
    input check, 2^20 machinery fwd / coset     0.37, 0.38 / 0.28 s
    leg, log_n 25 / 26 / 27                     0.03 / 0.06 / 0.11 .. 0.14 s
    leg, log_n 28  fwd, coset, inv / icoset     0.33 .. 0.34 / 0.22 s
    poly-eval, log_n 25 / 26 / 27 / 28          0.02 / 0.04 / 0.08 / 0.15 s
    extend (23,2) / (24,2) / (24,3) / (24,4)    0.04 / 0.05 / 0.10 / 0.20 s
All far below the 4.9 s of the largest oracle item, so no item is split.
"""
import random

import pytest
import torch

import ntt_split_ref as sr

pytestmark = pytest.mark.gpu

R = sr.R
SIZES = (25, 26, 27, 28)
SUB_LOG = 23                     # n2 = 2^23, n1 = 4 .. 32
LEGS = ("fwd", "coset", "inv", "icoset")
# (log_n, ext_bits) of the extend cases; N = 2^(log_n + ext_bits)
EXTEND = [(23, 2), (24, 2), (24, 3), (24, 4)]
# (log_n, ext_bits, coset generator, in place)
EXTEND_CASES = [(23, 2, 5, False), (23, 2, None, False),
                (24, 2, 5, False), (24, 2, 5, True),
                (24, 3, 5, False), (24, 4, 5, False)]
MACHINERY_LOG = 20
NEVER_SKIP = (25, 26)

R_TOP = R >> 192                 # 0x30644e72e131a029
I64 = torch.iinfo(torch.int64)
FILL = 0xa5a5a5a5a5a5a5a5 - (1 << 64)   # 0xa5 bytes as an int64


def limbs(v: int) -> list[int]:
    """Four little-endian 64-bit limbs as int64 values."""
    out = [(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]
    return [w - (1 << 64) if w >> 63 else w for w in out]


def planted(n: int):
    """(index, stored value): 0 and r - 1 at both ends and in each third."""
    return [(0, 0), (n - 1, R - 1), (n // 6, R - 1), (n // 6 + 1, 0),
            (n // 2, 0), (n // 2 + 1, R - 1), (5 * (n // 6) + 1, R - 1),
            (5 * (n // 6) + 2, 0)]


_vec = (None, None)  # (log_n, tensor): the last input vector; read-only


def drop_vec():
    global _vec
    _vec = (None, None)
    torch.cuda.empty_cache()


def room(log_n: int):
    """Skip (27 and 28 only) when the device has less free memory than the
    four vectors an item at 2^log_n needs."""
    need = 4 * (32 << log_n)
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if free < need:
        print(f"log_n {log_n}: {need} bytes needed, {free} of {total} free")
        if log_n not in NEVER_SKIP:
            pytest.skip(f"{free} bytes free, {need} needed")


def vec(log_n: int) -> torch.Tensor:
    """The input at 2^log_n: 4 << log_n int64 limbs on the device."""
    global _vec
    if _vec[0] != log_n:
        drop_vec()
        n = 1 << log_n
        gen = torch.Generator(device="cuda").manual_seed(8800 + log_n)
        x = torch.randint(I64.min, I64.max, (n, 4), dtype=torch.int64,
                          device="cuda", generator=gen)
        x[:, 3] = torch.randint(0, R_TOP, (n,), dtype=torch.int64,
                                device="cuda", generator=gen)
        for i, v in planted(n):
            x[i] = torch.tensor(limbs(v), dtype=torch.int64, device="cuda")
        _vec = (log_n, x.view(-1))
    return _vec[1]


def to_bytes(t: torch.Tensor) -> bytes:
    return t.cpu().numpy().tobytes()


def leg_args(log_n: int, leg: str):
    """(omega, inverse, coset_gen) of a leg, Montgomery bytes, as
    test_ntt_shapes_gpu.leg_args."""
    w = sr.ref.fr_root_of_unity(log_n)
    inverse = leg in ("inv", "icoset")
    if inverse:
        w = pow(w, -1, R)
    g = {"coset": sr.COSET_GEN, "icoset": pow(sr.COSET_GEN, -1, R)}.get(leg)
    return sr.enc(w), inverse, sr.enc(g) if g is not None else None


def run_leg(gpu, X: torch.Tensor, log_n: int, leg: str):
    """The transform under test, in place on X."""
    w, inverse, g = leg_args(log_n, leg)
    torch.cuda.empty_cache()  # the arena may grow
    torch.cuda.synchronize()
    gpu.ntt_device(X.data_ptr(), log_n, w, inverse=inverse, coset_gen=g)


def first_diff(a: torch.Tensor, b: torch.Tensor):
    """None when equal, else the first element index that differs."""
    if torch.equal(a, b):
        return None
    step = 4 << 20
    for lo in range(0, a.numel(), step):
        ne = a[lo:lo + step] != b[lo:lo + step]
        if bool(ne.any()):
            return (lo + int(ne.nonzero()[0])) // 4


@pytest.fixture(scope="module")
def ctx():
    from spectre_amd import SpectreGpu
    g = SpectreGpu([0])
    yield g
    drop_vec()
    g.close()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def be(ctx):
    return sr.DeviceBackend(ctx, torch)


def test_input_is_dense_and_below_r():
    log_n = 16
    n = 1 << log_n
    raw = to_bytes(vec(log_n))
    vals = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, 32 * n, 32)]
    assert max(vals) == R - 1 and min(vals) == 0
    assert all(vals[i] == v for i, v in planted(n))
    assert len(set(vals)) >= n - len(planted(n))
    # all four limbs are spread: the top limb over [0, R_TOP), the others
    # over 64 bits (n/2 expected, standard deviation 128)
    about_half = range(n // 2 - n // 32, n // 2 + n // 32)
    assert sum(v >> 192 > R_TOP // 2 for v in vals) in about_half
    for limb in range(3):
        assert sum((v >> (64 * limb + 63)) & 1 for v in vals) in about_half
    drop_vec()


@pytest.mark.parametrize("leg", ("fwd", "coset"))
def test_machinery_vs_oracle_at_2pow20(ctx, be, oracle, leg):
    log_n, n1 = MACHINERY_LOG, 4
    x = vec(log_n)
    X = x.clone()
    run_leg(ctx, X, log_n, leg)
    w, inverse, g = leg_args(log_n, leg)
    assert to_bytes(X) == oracle.ntt(to_bytes(x), log_n, w, inverse=inverse,
                                     coset_gen=g)
    form = sr.leg_form_mont(log_n, n1, leg)
    assert sr.mismatches(be, x, X, form) == []
    # and the strided compare sees one wrong limb of one element
    X.view(-1, 4)[n1 * 1234 + 3, 0] ^= 1
    assert sr.mismatches(be, x, X, form) == [3]


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("log_n", SIZES)
def test_leg_vs_split_reference(ctx, be, log_n, leg):
    if _vec[0] != log_n:
        drop_vec()
    room(log_n)
    x = vec(log_n)
    X = x.clone()
    if leg == "icoset":
        run_leg(ctx, X, log_n, "coset")
        run_leg(ctx, X, log_n, "icoset")
        assert first_diff(X, x) is None
        return
    run_leg(ctx, X, log_n, leg)
    form = sr.leg_form_mont(log_n, 1 << (log_n - SUB_LOG), leg)
    assert sr.mismatches(be, x, X, form) == []


@pytest.mark.parametrize("leg", ("fwd", "coset"))
@pytest.mark.parametrize("log_n", SIZES)
def test_outputs_vs_poly_eval(ctx, log_n, leg):
    """X[j] = x(g * w^j) at j = 0, 1, n/2, n - 1 and four seeded indices."""
    if _vec[0] != log_n:
        drop_vec()
    room(log_n)
    n = 1 << log_n
    x = vec(log_n)
    X = x.clone()
    run_leg(ctx, X, log_n, leg)
    rng = random.Random(8900 + log_n)
    js = [0, 1, n // 2, n - 1] + [rng.randrange(n) for _ in range(4)]
    w, g, _ = sr.leg_ints(log_n, leg)
    points = [sr.enc(g * pow(w, j, R)) for j in js]
    torch.cuda.synchronize()
    want = ctx.fr_poly_eval(x.data_ptr(), n, points)
    rows = X.view(-1, 4)
    got = [to_bytes(rows[j]) for j in js]
    assert got == want, [j for j, a, b in zip(js, got, want) if a != b]


@pytest.mark.parametrize("log_n,ext,g,in_place", EXTEND_CASES)
def test_extend_vs_coset_leg_of_the_padded_buffer(ctx, log_n, ext, g, in_place):
    big_log = log_n + ext
    if _vec[0] != log_n:
        drop_vec()
    room(big_log)
    n, big = 1 << log_n, 1 << big_log
    c = vec(log_n)
    w = sr.enc(sr.ref.fr_root_of_unity(big_log))
    gen = sr.enc(g) if g is not None else None
    Z = torch.zeros(4 * big, dtype=torch.int64, device="cuda")
    Z[:4 * n] = c
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    ctx.ntt_device(Z.data_ptr(), big_log, w, coset_gen=gen)
    # 0xa5 bytes wherever the call has to write; in place they are also the
    # tail behind the coefficients, which it must not read
    out = torch.full((4 * big,), FILL, dtype=torch.int64, device="cuda")
    if in_place:
        out[:4 * n] = c
    src = out if in_place else c
    torch.cuda.synchronize()
    ctx.ntt_extend_device(src.data_ptr(), log_n, ext, out.data_ptr(), w,
                          coset_gen=gen)
    assert first_diff(out, Z) is None
