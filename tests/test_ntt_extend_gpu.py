"""GPU checks of spectre_gpu_ntt_fr_extend_device and
spectre_gpu_fr_vec_mul_periodic.

Bit-exact means byte equality with the oracle's
ntt(coeffs + zeros, log_n + ext_bits, omega_ext, coset_gen=g). One module-wide
coefficient vector is generated once and sliced per shape; oracle results are
computed once per (shape, generator) and shared. Every shape is the smallest
that reaches one path of the extend pass (see SHAPES)."""
import importlib.util
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location(
    "bn254_ref", os.path.join(HERE, "golden", "bn254_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
R = ref.R
MONT_INV = pow(ref.MONT, -1, R)
FILL = b"\xa5" * 32

# (log_n, ext_bits); N = 2^(log_n + ext_bits)
SINGLE_PASS = [
    (0, 2), (0, 0),     # n = 1
    (1, 1),
    (3, 2),
    (2, 3),             # L' small, odd remaining level count
    (9, 3), (10, 2),    # N = 2^12: the radix-4 tile, odd / even remaining
    (12, 0),            # equals the plain coset call
]
TWO_PASS = [
    (11, 2),            # N = 2^13, split (1,12): first axis < ext_bits
    (12, 2), (13, 1),   # N = 2^14, split (2,12): L' = 1 and L' = 2
    (14, 2),            # N = 2^16
    (19, 2),            # N = 2^21, the smallest size on the balanced rule
]
FORCE3 = [(1, 2), (3, 2), (5, 2), (10, 2), (12, 2), (11, 3)]
GENS = ("five", "zeta", None)


def enc(v: int) -> bytes:
    return ref.to_mont_bytes(v % R, R)


def ints(data: bytes) -> list[int]:
    return [int.from_bytes(data[i:i + 32], "little") * MONT_INV % R
            for i in range(0, len(data), 32)]


def omega(log_n: int) -> bytes:
    return enc(ref.fr_root_of_unity(log_n))


def gen(name):
    """halo2's extended coset is zeta = 7^((r-1)/3), older forks' a plain
    generator; None is no coset factor."""
    if name is None:
        return None
    return enc(5 if name == "five" else pow(ref.FR_GEN, (R - 1) // 3, R))


@pytest.fixture(scope="module")
def coeffs(oracle):
    return oracle.gen_fr_vector(1 << 19, seed=6101)


_want = {}


def want(oracle, coeffs, log_n, ext, name):
    key = (log_n, ext, name)
    if key not in _want:
        n, big = 1 << log_n, 1 << (log_n + ext)
        _want[key] = oracle.ntt(coeffs[:32 * n] + bytes(32 * (big - n)),
                                log_n + ext, omega(log_n + ext),
                                coset_gen=gen(name))
    return _want[key]


def extend(gpu, src: bytes, log_n, ext, name, in_place=False, tail=FILL):
    """Upload src (n elements), extend, download N elements. In place, the
    N - n elements behind the coefficients are filled with `tail` first."""
    n, big = 1 << log_n, 1 << (log_n + ext)
    d_out = gpu.malloc(32 * big)
    if in_place:
        gpu.upload(d_out, src + tail * (big - n))
        d_src = d_out
    else:
        d_src = gpu.malloc(32 * n)
        gpu.upload(d_src, src)
    try:
        gpu.ntt_extend_device(d_src, log_n, ext, d_out, omega(log_n + ext),
                              coset_gen=gen(name))
        return gpu.download(d_out, 32 * big)
    finally:
        gpu.free(d_out)
        if not in_place:
            gpu.free(d_src)


@pytest.mark.parametrize("log_n,ext", SINGLE_PASS + TWO_PASS)
def test_extend_vs_oracle(gpu, oracle, coeffs, log_n, ext):
    src = coeffs[:32 << log_n]
    for name in GENS:
        got = extend(gpu, src, log_n, ext, name)
        assert got == want(oracle, coeffs, log_n, ext, name), name


def test_extend_without_extension_is_the_coset_call(gpu, oracle, coeffs):
    log_n = 12
    src = coeffs[:32 << log_n]
    for name in GENS:
        assert extend(gpu, src, log_n, 0, name) == gpu.ntt(
            src, log_n, omega(log_n), coset_gen=gen(name)), name


@pytest.mark.parametrize("log_n,ext", [(3, 2), (10, 2), (12, 2), (14, 2)])
def test_extend_in_place_never_reads_the_tail(gpu, oracle, coeffs, log_n, ext):
    """d_out == d_coeffs with 0xA5 bytes behind the coefficients: a single
    pass (small and radix-4 tile) and two passes."""
    src = coeffs[:32 << log_n]
    for name in GENS:
        got = extend(gpu, src, log_n, ext, name, in_place=True)
        assert got == want(oracle, coeffs, log_n, ext, name), name


@pytest.mark.parametrize("log_n,ext", [(3, 2), (11, 2), (12, 2)])
def test_extend_never_reads_or_writes_the_neighbour(gpu, oracle, coeffs,
                                                   log_n, ext):
    """Out of place from the first n elements of a 2n-element allocation
    whose second half is 0xA5: bit-exact, and all 2n elements unchanged."""
    n, big = 1 << log_n, 1 << (log_n + ext)
    src = coeffs[:32 * n] + FILL * n
    d_src = gpu.malloc(64 * n)
    d_out = gpu.malloc(32 * big)
    gpu.upload(d_src, src)
    for name in GENS:
        gpu.ntt_extend_device(d_src, log_n, ext, d_out, omega(log_n + ext),
                              coset_gen=gen(name))
        assert gpu.download(d_out, 32 * big) == want(oracle, coeffs, log_n,
                                                     ext, name), name
        assert gpu.download(d_src, 64 * n) == src, name
    gpu.free(d_src)
    gpu.free(d_out)


@pytest.mark.parametrize("log_n,ext", [(10, 2), (12, 2)])
def test_extend_round_trip(gpu, oracle, coeffs, log_n, ext):
    """extend, then the inverse-coset call with g^-1 at N: the coefficients
    followed by zeros."""
    n, big = 1 << log_n, 1 << (log_n + ext)
    src = coeffs[:32 * n]
    w_inv = oracle.fr_inv(omega(log_n + ext))
    for name in ("five", "zeta"):
        d = gpu.malloc(32 * big)
        gpu.upload(d, src + FILL * (big - n))
        gpu.ntt_extend_device(d, log_n, ext, d, omega(log_n + ext),
                              coset_gen=gen(name))
        gpu.ntt_device(d, log_n + ext, w_inv, inverse=True,
                       coset_gen=oracle.fr_inv(gen(name)))
        assert gpu.download(d, 32 * big) == src + bytes(32 * (big - n)), name
        gpu.free(d)


def test_extend_three_pass_forced_vs_oracle(oracle, coeffs):
    """The three-axis split forced at oracle-checkable sizes, in a fresh child
    process (the split rule is fixed when the context is created): (1,2)
    splits (1,1,1), (3,2) (2,2,1), (5,2) (3,2,2). Every generator, out of
    place; in place with a 0xA5 tail at (5,2) and (10,2)."""
    code = r'''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import pywrap as oracle
import test_ntt_extend_gpu as t
from spectre_amd import SpectreGpu
gpu = SpectreGpu([0])
coeffs = oracle.gen_fr_vector(1 << 12, seed=6102)
for log_n, ext in %r:
    src = coeffs[:32 << log_n]
    for name in t.GENS:
        w = t.want(oracle, coeffs, log_n, ext, name)
        assert t.extend(gpu, src, log_n, ext, name) == w, (log_n, ext, name)
        if (log_n, ext) in ((5, 2), (10, 2)):
            assert t.extend(gpu, src, log_n, ext, name, in_place=True) == w, (
                log_n, ext, name, "in place")
gpu.close()
print("extend legs ok")
''' % (REPO, os.path.join(REPO, "oracle"), HERE, FORCE3)
    env = dict(os.environ, SPECTRE_NTT_FORCE3="1")
    r = subprocess.run([sys.executable, "-c", code], env=env,
                       capture_output=True, text=True, timeout=300)
    assert "extend legs ok" in r.stdout, r.stdout + r.stderr


def test_quotient_chain_at_the_extended_shape(gpu, oracle):
    """Evaluations -> inverse NTT at n -> extend to N = 4n -> gate expression
    at N with rot_scale = 4 -> multiply by the period-4 table -> inverse
    coset NTT at N, all on the device, against the same chain through the
    oracle's NTTs and Python integers."""
    log_n, ext = 8, 2
    n, big = 1 << log_n, 1 << (log_n + ext)
    w, w_ext = omega(log_n), omega(log_n + ext)
    zeta = gen("zeta")
    cols = [oracle.gen_fr_vector(n, 6200 + i) for i in range(3)]
    table = oracle.gen_fr_vector(1 << ext, 6210)

    d_cols = []
    for c in cols:
        d = gpu.malloc(32 * big)
        gpu.upload(d, c + FILL * (big - n))
        gpu.ntt_device(d, log_n, oracle.fr_inv(w), inverse=True)
        gpu.ntt_extend_device(d, log_n, ext, d, w_ext, coset_gen=zeta)
        d_cols.append(d)
    d_h = gpu.malloc(32 * big)
    G = gpu
    # q * (a + b*c - d): q = col 0, a, b = col 1 at rotations 0, 1,
    # c, d = col 2 at rotations 2, 3
    flex = [(G.GATE_COL, 0, 0),
            (G.GATE_COL, 1, 0), (G.GATE_COL, 1, 1), (G.GATE_COL, 2, 2),
            (G.GATE_MUL, 0, 0), (G.GATE_ADD, 0, 0),
            (G.GATE_COL, 2, 3), (G.GATE_SUB, 0, 0),
            (G.GATE_MUL, 0, 0)]
    G.gate_eval(d_cols, b"", flex, big, rot_scale=1 << ext, d_out=d_h)
    gpu.fr_vec_mul_periodic(d_h, table, d_h, big)
    gpu.ntt_device(d_h, log_n + ext, oracle.fr_inv(w_ext), inverse=True,
                   coset_gen=oracle.fr_inv(zeta))
    got = gpu.download(d_h, 32 * big)
    for d in d_cols + [d_h]:
        gpu.free(d)

    ev = []
    for c in cols:
        co = oracle.ntt(c, log_n, oracle.fr_inv(w), inverse=True)
        ev.append(ints(oracle.ntt(co + bytes(32 * (big - n)), log_n + ext,
                                  w_ext, coset_gen=zeta)))
    tab = ints(table)
    rs = 1 << ext
    h = [ev[0][i] * (ev[1][i] + ev[1][(i + rs) % big] * ev[2][(i + 2 * rs) % big]
                     - ev[2][(i + 3 * rs) % big]) * tab[i % len(tab)] % R
         for i in range(big)]
    assert got == oracle.ntt(b"".join(enc(v) for v in h), log_n + ext,
                             oracle.fr_inv(w_ext), inverse=True,
                             coset_gen=oracle.fr_inv(zeta))


@pytest.mark.parametrize("n", [4097, 1])
def test_fr_vec_mul_periodic_vs_oracle(gpu, oracle, coeffs, n):
    a = coeffs[:32 * n]
    d_a = gpu.malloc(32 * n)
    d_o = gpu.malloc(32 * n)
    for period in (1, 4, 64):
        table = oracle.gen_fr_vector(period, 6300 + period)
        exp = b"".join(
            oracle.fr_mul(a[32 * i:32 * i + 32],
                          table[32 * (i % period):32 * (i % period) + 32])
            for i in range(n))
        gpu.upload(d_a, a)
        gpu.fr_vec_mul_periodic(d_a, table, d_o, n)
        assert gpu.download(d_o, 32 * n) == exp, period
        assert gpu.download(d_a, 32 * n) == a, period
        gpu.fr_vec_mul_periodic(d_a, table, d_a, n)  # aliased
        assert gpu.download(d_a, 32 * n) == exp, (period, "aliased")
    gpu.upload(d_o, FILL * n)
    gpu.fr_vec_mul_periodic(d_a, oracle.gen_fr_vector(4, 1), d_o, 0)  # n = 0
    assert gpu.download(d_o, 32 * n) == FILL * n
    gpu.free(d_a)
    gpu.free(d_o)


def test_error_paths_leave_the_context_usable(gpu, oracle, coeffs):
    log_n, ext = 3, 2
    n, big = 1 << log_n, 1 << (log_n + ext)
    src = coeffs[:32 * n]
    w = omega(log_n + ext)
    d = gpu.malloc(32 * 2 * big)
    gpu.upload(d, src + FILL * (2 * big - n))

    def still_right():
        assert extend(gpu, src, log_n, ext, "five") == want(
            oracle, coeffs, log_n, ext, "five")
        table = oracle.gen_fr_vector(4, 6400)
        gpu.fr_vec_mul_periodic(d, table, d + 32 * big, n)
        assert gpu.download(d + 32 * big, 32 * n) == b"".join(
            oracle.fr_mul(src[32 * i:32 * i + 32],
                          table[32 * (i % 4):32 * (i % 4) + 32])
            for i in range(n))

    bad_extend = [
        (0, d + 32 * big),             # null source
        (d, 0),                        # null destination
        (d, d + 32),                   # destination starts inside the source
        (d, d + 32 * (n - 1)),         # ... at its last element
        (d + 32 * (big - 1), d),       # source is the destination's last element
        (d + 32, d),                   # in place but shifted
    ]
    for d_src, d_dst in bad_extend:
        with pytest.raises(RuntimeError, match="rc=-1"):
            gpu.ntt_extend_device(d_src, log_n, ext, d_dst, w)
        still_right()
    # adjacent ranges are disjoint: allowed
    gpu.ntt_extend_device(d, log_n, ext, d + 32 * n, w, coset_gen=gen("five"))
    assert gpu.download(d + 32 * n, 32 * big) == want(oracle, coeffs, log_n,
                                                      ext, "five")
    gpu.upload(d, src)
    for ln, e in ((27, 2), (29, 0), (0, 29)):
        with pytest.raises(RuntimeError, match="rc=-3"):
            gpu.ntt_extend_device(d, ln, e, d, w)
        still_right()
    for period in (0, 3, 128):
        with pytest.raises(RuntimeError, match="rc=-1"):
            gpu.fr_vec_mul_periodic(d, bytes(32 * period), d, n)
        still_right()
    for d_a, d_o in ((0, d), (d, 0)):
        with pytest.raises(RuntimeError, match="rc=-1"):
            gpu.fr_vec_mul_periodic(d_a, bytes(32), d_o, n)
        still_right()
    gpu.free(d)
