"""spectre_gpu_ntt_fr(_device) against the oracle at every pass shape the
default split rule produces up to 2^24.

k_ntt_pass behaves by tile size, radix, position (only / first / middle /
last pass) and stride, and ntt_split fixes those per log_n; SHAPES is every
log_n whose split has a pass of its own, and tests/test_ntt_split.py fails
when the rule reaches a pass class that SHAPES does not.

Bit-exact means byte equality with oracle.ntt on the same input. The four
legs are forward, inverse, forward coset (g = 5) and inverse coset (g = 5^-1).
log_n 1..22 check all four through ntt_device on a device buffer; HOST_ENTRY
sizes repeat them through the host-pointer gpu.ntt. At 23 and 24 the two
coset legs are compared with the oracle (between them: the coset multiply on
load, n^-1, and the coset multiply on the scattered store) and the plain pair
is a device-resident round trip, so each size costs two oracle transforms.

Input: one seeded 2^20-element chunk per module, sliced per size. Above 2^20
the vector is copies of the chunk, each rotated by another odd element count:
as cheap as plain repetition, but a plainly repeated chunk is periodic, and
the DFT of a vector of period 2^20 at 2^24 is zero at 15 outputs of 16, where
no wrong factor shows. EDGE sizes also run the Fr catalogue of
edge_operands.py (0, 1, r - 1, ...) cycled over the vector, for the add / sub
corner cases of the butterflies, and one size the all-zero vector.

The module runs in the session context: its plan cache ends up holding every
(omega, log_n) of the sweep at once.

Oracle results are kept per (data, log_n, leg) up to 2^21, the sizes that
more than one test reads; above, each is read once and dropped.

Wall time per item on an MI355X host (16 oracle threads), pytest
--durations, the whole module 24 s:
    log_n <= 19          0.10 s at the most
    20                   0.17 .. 0.25 s
    21                   0.41 .. 0.53 s
    22                   0.86 .. 1.13 s
    23  coset / icoset   2.50 / 2.36 s
    24  coset / icoset   4.89 / 4.60 s
    23, 24 round trip    0.34, 0.61 s
2^23 and 2^24 are the largest items because 2^24 is the smallest size at which
the (12,12) split exists; nearly all of their time is the oracle's. None is
near the 20 s at which an item would compare only a prefix.
"""
import importlib.util
import os

import pytest

import edge_operands as eo

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "bn254_ref", os.path.join(HERE, "golden", "bn254_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
R = ref.R

FULL = tuple(range(1, 23))       # four legs against the oracle
LARGE = (23, 24)                 # coset legs against the oracle + round trip
SHAPES = FULL + LARGE
# odd small tile, both lone-radix-2 tiles, a two-pass and a balanced size
HOST_ENTRY = (5, 9, 11, 15, 21)
EDGE = (11, 15)                  # single pass, two passes
ZERO = 13
LEGS = ("fwd", "inv", "coset", "icoset")
CHUNK_LOG = 20
RETAIN_LOG = 21


def enc(v: int) -> bytes:
    return ref.to_mont_bytes(v % R, R)


def leg_args(log_n: int, leg: str):
    """(omega, inverse, coset_gen) of a leg, Montgomery bytes."""
    w = ref.fr_root_of_unity(log_n)
    inverse = leg in ("inv", "icoset")
    if inverse:
        w = pow(w, -1, R)
    g = {"coset": 5, "icoset": pow(5, -1, R)}.get(leg)
    return enc(w), inverse, enc(g) if g is not None else None


_chunk = None
_big = (None, None)  # (log_n, vector): the last vector above the chunk size


@pytest.fixture(scope="module", autouse=True)
def _data(oracle):
    global _chunk, _big
    _chunk = oracle.gen_fr_vector(1 << CHUNK_LOG, seed=7301)
    yield
    _chunk = None
    _big = (None, None)
    _want.clear()


def vec(log_n: int) -> bytes:
    global _big
    if log_n <= CHUNK_LOG:
        return _chunk[:32 << log_n]
    if _big[0] != log_n:
        parts = []
        for j in range(1 << (log_n - CHUNK_LOG)):
            cut = 32 * ((j * 40503) % (1 << CHUNK_LOG))
            parts.append(_chunk[cut:] + _chunk[:cut])
        _big = (log_n, b"".join(parts))
    return _big[1]


def edge_vec(log_n: int) -> bytes:
    sp = eo.specials(R)
    reps = (1 << log_n) // len(sp) + 1
    return (eo.imgs_bytes(sp) * reps)[:32 << log_n]


_want = {}


def want(oracle, kind: str, data: bytes, log_n: int, leg: str) -> bytes:
    key = (kind, log_n, leg)
    if key in _want:
        return _want[key]
    w, inverse, g = leg_args(log_n, leg)
    out = oracle.ntt(data, log_n, w, inverse=inverse, coset_gen=g)
    if log_n <= RETAIN_LOG:
        _want[key] = out
    return out


def first_diff(got: bytes, exp: bytes):
    """None when equal, else (element index, got, expected) of the first
    element that differs: a failure prints 64 bytes, not the vectors."""
    if got == exp:
        return None
    if len(got) != len(exp):
        return ("length", len(got), len(exp))
    step = 1 << 20
    for lo in range(0, len(exp), step):
        if got[lo:lo + step] != exp[lo:lo + step]:
            for i in range(lo, min(lo + step, len(exp)), 32):
                if got[i:i + 32] != exp[i:i + 32]:
                    return (i // 32, got[i:i + 32].hex(), exp[i:i + 32].hex())


def on_device(gpu, data: bytes, log_n: int, legs) -> bytes:
    """Upload, run the legs in order in place, download."""
    d = gpu.malloc(len(data))
    try:
        gpu.upload(d, data)
        for leg in legs:
            w, inverse, g = leg_args(log_n, leg)
            gpu.ntt_device(d, log_n, w, inverse=inverse, coset_gen=g)
        return gpu.download(d, len(data))
    finally:
        gpu.free(d)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("log_n", FULL)
def test_device_vs_oracle(gpu, oracle, log_n, leg):
    a = vec(log_n)
    got = on_device(gpu, a, log_n, [leg])
    assert first_diff(got, want(oracle, "seeded", a, log_n, leg)) is None


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("log_n", HOST_ENTRY)
def test_host_entry_vs_oracle(gpu, oracle, log_n, leg):
    a = vec(log_n)
    w, inverse, g = leg_args(log_n, leg)
    got = gpu.ntt(a, log_n, w, inverse=inverse, coset_gen=g)
    assert first_diff(got, want(oracle, "seeded", a, log_n, leg)) is None


@pytest.mark.parametrize("leg", ("coset", "icoset"))
@pytest.mark.parametrize("log_n", LARGE)
def test_large_coset_legs_vs_oracle(gpu, oracle, log_n, leg):
    a = vec(log_n)
    got = on_device(gpu, a, log_n, [leg])
    assert first_diff(got, want(oracle, "seeded", a, log_n, leg)) is None


@pytest.mark.parametrize("log_n", LARGE)
def test_large_plain_round_trip(gpu, log_n):
    a = vec(log_n)
    assert first_diff(on_device(gpu, a, log_n, ["fwd", "inv"]), a) is None


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("log_n", EDGE)
def test_edge_operands_vs_oracle(gpu, oracle, log_n, leg):
    a = edge_vec(log_n)
    assert len(eo.specials(R)) > 32 and a[:32] == bytes(32)
    got = on_device(gpu, a, log_n, [leg])
    assert first_diff(got, want(oracle, "edge", a, log_n, leg)) is None


@pytest.mark.parametrize("leg", LEGS)
def test_zero_vector_stays_zero(gpu, leg):
    zeros = bytes(32 << ZERO)
    assert first_diff(on_device(gpu, zeros, ZERO, [leg]), zeros) is None
