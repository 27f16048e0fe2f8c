"""GPU checks of spectre_gpu_fr_poly_eval / spectre_gpu_fr_poly_div_linear.

The reference is plain Python integers (tests/golden/bn254_ref.py, loaded by
path): Horner for a(x), and the top-down recurrence q[i] = a[i+1] + z q[i+1]
for the quotient by (X - z); every comparison is byte-exact. One module-wide
coefficient vector is generated once and sliced per case. Each test owns a
context, because it changes the tile, and restores the default before closing
it."""
import ctypes
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "bn254_ref", os.path.join(HERE, "golden", "bn254_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
R = ref.R
MONT_INV = pow(ref.MONT, -1, R)

N_LEVELS = 256 * 256 + 1    # tile 256: 65 537 -> 257 -> 2 -> 1
N_MAX = N_LEVELS + 300      # the tile-independence size
ZERO = bytes(32)
FILL = b"\xa5" * 32


def ints(data: bytes) -> list[int]:
    return [int.from_bytes(data[i:i + 32], "little") * MONT_INV % R
            for i in range(0, len(data), 32)]


def enc(v: int) -> bytes:
    return ref.to_mont_bytes(v % R, R)


def mont(vals) -> bytes:
    return b"".join(enc(v) for v in vals)


def horner(a, x: int) -> int:
    s = 0
    for c in reversed(a):
        s = (s * x + c) % R
    return s


def quotient(a, z: int):
    """(q, rem) with a(X) = (X - z) q(X) + rem and len(q) == len(a)."""
    q = [0] * len(a)
    for i in range(len(a) - 2, -1, -1):
        q[i] = (a[i + 1] + z * q[i + 1]) % R
    rem = (a[0] + z * q[0]) % R if a else 0
    return q, rem


@pytest.fixture(scope="module")
def data(oracle):
    a_b = oracle.gen_fr_vector(N_MAX, seed=5201)
    rnd = ints(oracle.gen_fr_vector(16, seed=5202))
    return {"a_b": a_b, "a": ints(a_b), "rnd": rnd,
            "b_b": oracle.gen_fr_vector(3 * 1024 + 4, seed=5203)}


@pytest.fixture
def fresh_gpu():
    from spectre_amd import SpectreGpu
    g = SpectreGpu([0])
    yield g
    g.set_fr_scan_tile(0)
    g.close()


def tile_in_force(tile: int) -> int:
    from spectre_amd import ffi
    return tile or ffi.fr_scan_tile_default()


def sizes(T: int) -> list[int]:
    return sorted({0, 1, 2, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5})


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
        return self.g.download(p, 32 * n) if n else b""

    def free(self):
        for p in self.ptrs:
            self.g.free(p)
        self.ptrs = []


def gpu_eval(g, a_b: bytes, points) -> list[bytes]:
    n = len(a_b) // 32
    d = Dev(g)
    d_a = d.put(a_b)
    out = g.fr_poly_eval(d_a, n, [enc(x) for x in points])
    assert d.get(d_a, n) == a_b, "poly_eval wrote its input"
    d.free()
    return out


def gpu_div(g, a_b: bytes, z: int, in_place: bool = False):
    """Returns (q bytes, rem bytes). Out of place, the output buffer has one
    element more than n, which has to stay untouched, like the input."""
    n = len(a_b) // 32
    d = Dev(g)
    d_a = d.put(a_b)
    d_q = d_a if in_place else d.put(FILL * (n + 1))
    rem = g.fr_poly_div_linear(d_a, enc(z), d_q, n)
    q = d.get(d_q, n)
    if not in_place:
        assert d.get(d_a, n) == a_b, "division wrote its input"
        assert d.get(d_q, n + 1)[32 * n:] == FILL, "division wrote past n"
    d.free()
    return q, rem


def check_div(g, data, n: int, z: int, what: str):
    q, rem = gpu_div(g, data["a_b"][:32 * n], z)
    want_q, want_rem = quotient(data["a"][:n], z)
    assert q == mont(want_q), what
    assert rem == enc(want_rem), what


def test_reference_sanity(oracle, data):
    n = 777
    a = data["a"][:n]
    z, r = data["rnd"][0], data["rnd"][1]
    q, rem = quotient(a, z)
    assert q[n - 1] == 0
    assert rem == horner(a, z)
    assert horner(a, r) == ((r - z) * horner(q, r) + rem) % R
    x_b, y_b = data["a_b"][:32], data["a_b"][32:64]
    assert oracle.fr_mul(x_b, y_b) == enc(data["a"][0] * data["a"][1])


@pytest.mark.parametrize("tile", [256, 0])
def test_sizes(fresh_gpu, data, tile):
    fresh_gpu.set_fr_scan_tile(tile)
    x, z = data["rnd"][2], data["rnd"][3]
    for n in sizes(tile_in_force(tile)):
        got = gpu_eval(fresh_gpu, data["a_b"][:32 * n], [x])
        assert got == [enc(horner(data["a"][:n], x))], f"eval n={n}"
        check_div(fresh_gpu, data, n, z, f"div n={n}")


def test_three_levels(fresh_gpu, data):
    """Tile 256 and n = 256*256 + 1: partial vectors of 257, 2 and 1
    elements, so a middle level has more than one tile above it."""
    fresh_gpu.set_fr_scan_tile(256)
    n = N_LEVELS
    pts = data["rnd"][4:7]
    got = gpu_eval(fresh_gpu, data["a_b"][:32 * n], pts)
    assert got == [enc(horner(data["a"][:n], x)) for x in pts]
    check_div(fresh_gpu, data, n, data["rnd"][7], "three levels")


def test_tile_independence(fresh_gpu, data):
    n = N_MAX
    pts = data["rnd"][:8]
    z = data["rnd"][8]
    want_eval = [enc(horner(data["a"], x)) for x in pts]
    want_q, want_rem = quotient(data["a"], z)
    want_div = (mont(want_q), enc(want_rem))
    for tile in (256, 512, 0):
        fresh_gpu.set_fr_scan_tile(tile)
        assert gpu_eval(fresh_gpu, data["a_b"], pts) == want_eval, \
            f"tile {tile}"
        assert gpu_div(fresh_gpu, data["a_b"], z) == want_div, f"tile {tile}"


def test_multi_point(fresh_gpu, data):
    x = data["rnd"][9]
    w = ref.fr_root_of_unity(12)
    pts = [0, 1, R - 1, x, x, x * w % R, x * pow(w, -1, R) % R,
           data["rnd"][10]]
    for tile in (256, 0):
        fresh_gpu.set_fr_scan_tile(tile)
        n = 3 * tile_in_force(tile) + 5
        a_b, a = data["a_b"][:32 * n], data["a"][:n]
        single = [gpu_eval(fresh_gpu, a_b, [p])[0] for p in pts]
        assert single == [enc(horner(a, p)) for p in pts]
        assert single[0] == enc(a[0]) and single[3] == single[4]
        for k in range(1, 9):
            assert gpu_eval(fresh_gpu, a_b, pts[:k]) == single[:k], \
                f"npoints {k} tile {tile}"


def test_special_z(fresh_gpu, data):
    for tile in (256, 0):
        fresh_gpu.set_fr_scan_tile(tile)
        n = 3 * tile_in_force(tile) + 5
        a_b = data["a_b"][:32 * n]
        q, rem = gpu_div(fresh_gpu, a_b, 0)
        assert q == a_b[32:] + ZERO, "z = 0: q[i] = a[i+1]"
        assert rem == a_b[:32], "z = 0: rem = a[0]"
        for z in (1, R - 1):
            check_div(fresh_gpu, data, n, z, f"z={z} tile {tile}")


def test_exact_root(fresh_gpu, data):
    """a = (X - z) b built on the host: remainder zero and the quotient is
    b, which is halo2's actual use of kate_division."""
    z = data["rnd"][11]
    for tile in (256, 0):
        fresh_gpu.set_fr_scan_tile(tile)
        m = 3 * tile_in_force(tile) + 4
        b_b = data["b_b"][:32 * m]
        b = ints(b_b)
        a = [(-z * b[0]) % R]
        a += [(b[i - 1] - z * b[i]) % R for i in range(1, m)]
        a.append(b[m - 1])
        q, rem = gpu_div(fresh_gpu, mont(a), z)
        assert rem == ZERO
        assert q[:32 * m] == b_b
        assert q[32 * m:] == ZERO


def test_aliasing(fresh_gpu, data):
    z = data["rnd"][12]
    for tile, n in ((256, 3 * 256 + 5), (0, 3 * tile_in_force(0) + 5),
                    (256, N_LEVELS)):
        fresh_gpu.set_fr_scan_tile(tile)
        a_b = data["a_b"][:32 * n]
        out_of_place = gpu_div(fresh_gpu, a_b, z)  # checks d_a untouched
        assert gpu_div(fresh_gpu, a_b, z, in_place=True) == out_of_place
        want_q, want_rem = quotient(data["a"][:n], z)
        assert out_of_place == (mont(want_q), enc(want_rem))


def test_eval_and_division_agree_on_device(fresh_gpu, data):
    """a(r) = q(r) (r - z) + rem from GPU outputs alone."""
    g = fresh_gpu
    n = 3 * tile_in_force(0) + 5
    z, r = data["rnd"][13], data["rnd"][14]
    d = Dev(g)
    d_a = d.put(data["a_b"][:32 * n])
    d_q = d.put(FILL * n)
    rem = g.fr_poly_div_linear(d_a, enc(z), d_q, n)
    a_r = g.fr_poly_eval(d_a, n, [enc(r)])[0]
    q_r = g.fr_poly_eval(d_q, n, [enc(r)])[0]
    d.free()
    assert ints(a_r)[0] == (ints(q_r)[0] * (r - z) + ints(rem)[0]) % R


def test_pipeline_division_commit_and_intt_eval(fresh_gpu, oracle, data):
    """Coefficients on the device -> in-place division -> MSM equals the
    commitment of the host-computed quotient uploaded; and evaluating an
    inverse-NTT'd buffer at omega^5 gives back row 5 of the Lagrange data."""
    g = fresh_gpu
    log_n = 12
    n = 1 << log_n
    _, bases = oracle.gen_msm_inputs(n, seed=5204, fast=True)
    z = data["rnd"][15]
    a_b, a = data["a_b"][:32 * n], data["a"][:n]
    want_q, want_rem = quotient(a, z)
    d = Dev(g)
    d_bases = d.put(bases)
    d_a = d.put(a_b)
    d_host = d.put(mont(want_q))
    rem = g.fr_poly_div_linear(d_a, enc(z), d_a, n)
    got = g.msm_device(d_bases, d_a, n, canonical=False)
    want = g.msm_device(d_bases, d_host, n, canonical=False)
    assert rem == enc(want_rem)
    assert got == want, "commitments differ"
    assert got != bytes(64)
    w = ref.fr_root_of_unity(log_n)
    d_l = d.put(a_b)  # read as Lagrange values
    g.ntt_device(d_l, log_n, enc(pow(w, -1, R)), inverse=True)
    at_row5 = g.fr_poly_eval(d_l, n, [enc(pow(w, 5, R))])
    d.free()
    assert at_row5 == [a_b[32 * 5:32 * 6]]


def test_error_paths(fresh_gpu, data):
    g = fresh_gpu
    n = 300
    a_b, a = data["a_b"][:32 * n], data["a"][:n]
    x = data["rnd"][0]
    d = Dev(g)
    d_a = d.put(a_b)
    d_q = d.put(FILL * n)
    too_many = (1 << 28) + 1
    with pytest.raises(RuntimeError, match="2\\^28"):
        g.fr_poly_eval(d_a, too_many, [enc(x)])
    with pytest.raises(RuntimeError, match="2\\^28"):
        g.fr_poly_div_linear(d_a, enc(x), d_q, too_many)
    with pytest.raises(RuntimeError, match="null"):
        g.fr_poly_eval(0, n, [enc(x)])
    with pytest.raises(RuntimeError, match="null"):
        g.fr_poly_div_linear(0, enc(x), d_q, n)
    with pytest.raises(RuntimeError, match="null"):
        g.fr_poly_div_linear(d_a, enc(x), 0, n)
    # null host pointers cannot be reached through the mirror
    lib, ctx = g._lib, g._ctx
    buf = (ctypes.c_uint8 * 32)()
    for pts, out in ((None, buf), (buf, None)):
        assert lib.spectre_gpu_fr_poly_eval(
            ctx, 0, ctypes.c_void_p(d_a), n, pts, 1, out) != 0
        assert b"null" in lib.spectre_gpu_last_error()
    assert lib.spectre_gpu_fr_poly_div_linear(
        ctx, 0, ctypes.c_void_p(d_a), None, ctypes.c_void_p(d_q), n,
        buf) != 0
    assert b"null" in lib.spectre_gpu_last_error()
    with pytest.raises(RuntimeError, match="npoints"):
        g.fr_poly_eval(d_a, n, [])
    with pytest.raises(RuntimeError, match="npoints"):
        g.fr_poly_eval(d_a, n, [enc(x)] * 9)
    with pytest.raises(RuntimeError, match="invalid ctx/device"):
        g.fr_poly_eval(d_a, n, [enc(x)], dev=7)
    with pytest.raises(RuntimeError, match="invalid ctx/device"):
        g.fr_poly_div_linear(d_a, enc(x), d_q, n, dev=7)
    # nothing was written by the rejected calls, and valid calls still work
    assert d.get(d_q, n) == FILL * n
    assert g.fr_poly_eval(d_a, n, [enc(x)]) == [enc(horner(a, x))]
    # a null remainder pointer is allowed
    assert lib.spectre_gpu_fr_poly_div_linear(
        ctx, 0, ctypes.c_void_p(d_a), (ctypes.c_uint8 * 32).from_buffer_copy(
            enc(x)), ctypes.c_void_p(d_q), n, None) == 0
    want_q, want_rem = quotient(a, x)
    assert d.get(d_q, n) == mont(want_q)
    assert g.fr_poly_div_linear(d_a, enc(x), d_q, n) == enc(want_rem)
    d.free()
