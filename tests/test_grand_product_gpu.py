"""GPU checks of spectre_gpu_fr_batch_invert / spectre_gpu_fr_grand_product.

The reference is plain Python integers (tests/golden/bn254_ref.py, loaded by
path), cross-checked against the C oracle on a few elements; every comparison
is byte-exact. One module-wide input pair and its running products are
computed once and sliced per case. Each test owns a context, because it
changes the tile, and restores the default before closing it."""
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

N_CHUNKS = 256 * 256 + 1    # 257 tile products at tile 256: two chunks
N_MAX = N_CHUNKS + 300      # the tile-independence size
ZERO = bytes(32)


def ints(data: bytes) -> list[int]:
    return [ref.from_mont_bytes(data[i:i + 32], R)
            for i in range(0, len(data), 32)]


def mont(vals) -> bytes:
    return b"".join(ref.to_mont_bytes(v, R) for v in vals)


def inv(x: int) -> int:
    return pow(x, -1, R) if x else 0


def running(ratios) -> list[int]:
    """cum[i] = prod_{j<i} ratios[j], len(ratios) + 1 entries."""
    cum, acc = [1], 1
    for r in ratios:
        acc = acc * r % R
        cum.append(acc)
    return cum


@pytest.fixture(scope="module")
def data(oracle):
    num_b = oracle.gen_fr_vector(N_MAX, seed=4101)
    den_b = oracle.gen_fr_vector(N_MAX, seed=4102)
    num, den = ints(num_b), ints(den_b)
    assert all(den), "seeded denominators are expected to be nonzero"
    den_inv = [inv(d) for d in den]
    return {
        "num_b": num_b, "den_b": den_b, "num": num, "den": den,
        "den_inv": den_inv,
        "cum_ratio": running(a * b % R for a, b in zip(num, den_inv)),
        "cum_num": running(num),
        "z0": ints(oracle.gen_fr_vector(1, seed=4103))[0],
    }


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
    return sorted({1, 2, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5})


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


def gpu_invert(g, xs_b: bytes, in_place: bool = False) -> bytes:
    n = len(xs_b) // 32
    d = Dev(g)
    d_in = d.put(xs_b)
    d_out = d_in if in_place else d.put(b"\xa5" * len(xs_b))
    g.fr_batch_invert(d_in, d_out, n)
    out = d.get(d_out, n)
    if not in_place:
        assert d.get(d_in, n) == xs_b, "batch invert wrote its input"
    d.free()
    return out


def gpu_product(g, num_b: bytes, den_b, z0, alias=None):
    """Returns (z bytes, out_last bytes). alias: None, "num" or "den"."""
    n = len(num_b) // 32
    d = Dev(g)
    d_num = d.put(num_b)
    d_den = d.put(den_b) if den_b is not None else None
    d_z = {None: None, "num": d_num, "den": d_den}[alias]
    if d_z is None:
        d_z = d.put(b"\xa5" * len(num_b))
    last = g.fr_grand_product(d_num, d_den,
                              None if z0 is None else ref.to_mont_bytes(z0, R),
                              d_z, n)
    z = d.get(d_z, n)
    d.free()
    return z, last


def want_product(data, n: int, with_den: bool, z0):
    cum = data["cum_ratio"] if with_den else data["cum_num"]
    s = 1 if z0 is None else z0
    return (mont(s * c % R for c in cum[:n]),
            ref.to_mont_bytes(s * cum[n] % R, R))


def test_reference_matches_oracle(oracle, data):
    for i in (0, 1, 2, 777, N_MAX - 1):
        x_b = data["den_b"][32 * i:32 * i + 32]
        y_b = data["num_b"][32 * i:32 * i + 32]
        assert oracle.fr_inv(x_b) == ref.to_mont_bytes(data["den_inv"][i], R)
        assert oracle.fr_mul(x_b, y_b) == ref.to_mont_bytes(
            data["den"][i] * data["num"][i] % R, R)


@pytest.mark.parametrize("tile", [256, 0])
def test_batch_invert_sizes(fresh_gpu, data, tile):
    fresh_gpu.set_fr_scan_tile(tile)
    for n in sizes(tile_in_force(tile)):
        got = gpu_invert(fresh_gpu, data["den_b"][:32 * n])
        assert got == mont(data["den_inv"][:n]), f"n={n}"


@pytest.mark.parametrize("tile", [256, 0])
def test_batch_invert_planted_zeros(fresh_gpu, data, tile):
    fresh_gpu.set_fr_scan_tile(tile)
    T = tile_in_force(tile)
    n = 3 * T + 5
    zeros = {0, T - 1, T, n - 1} | set(range(2 * T, 3 * T))
    xs = [0 if i in zeros else x for i, x in enumerate(data["den"][:n])]
    got = gpu_invert(fresh_gpu, mont(xs))
    out = ints(got)
    for i in range(n):
        if i in zeros:
            assert got[32 * i:32 * i + 32] == ZERO, f"zero at {i} moved"
        else:
            assert xs[i] * out[i] % R == 1, f"x * out != 1 at {i}"
    assert got == mont(inv(x) for x in xs)


def test_batch_invert_in_place(fresh_gpu, data):
    for tile in (256, 0):
        fresh_gpu.set_fr_scan_tile(tile)
        n = 3 * tile_in_force(tile) + 5
        got = gpu_invert(fresh_gpu, data["den_b"][:32 * n], in_place=True)
        assert got == mont(data["den_inv"][:n])


@pytest.mark.parametrize("tile", [256, 0])
def test_grand_product_forms(fresh_gpu, data, tile):
    fresh_gpu.set_fr_scan_tile(tile)
    for n in [0] + sizes(tile_in_force(tile)):
        for with_den in (True, False):
            for z0 in (None, data["z0"]):
                z, last = gpu_product(
                    fresh_gpu, data["num_b"][:32 * n],
                    data["den_b"][:32 * n] if with_den else None, z0)
                want_z, want_last = want_product(data, n, with_den, z0)
                what = f"n={n} den={with_den} z0={z0 is not None}"
                assert z == want_z, what
                assert last == want_last, what
    # n = 0 hands the seed back
    _, last = gpu_product(fresh_gpu, b"", None, data["z0"])
    assert last == ref.to_mont_bytes(data["z0"], R)
    _, last = gpu_product(fresh_gpu, b"", None, None)
    assert last == ref.to_mont_bytes(1, R)


def test_grand_product_level_two_chunk_loop(fresh_gpu, data):
    """Tile 256 and n = 256*256 + 1: 257 tile products, so the single
    workgroup of the middle launch loops twice and carries between chunks."""
    fresh_gpu.set_fr_scan_tile(256)
    n = N_CHUNKS
    z, last = gpu_product(fresh_gpu, data["num_b"][:32 * n],
                          data["den_b"][:32 * n], data["z0"])
    want_z, want_last = want_product(data, n, True, data["z0"])
    assert z == want_z
    assert last == want_last


def test_tile_independence(fresh_gpu, data):
    n = N_MAX
    want = want_product(data, n, True, None)
    want_inv = mont(data["den_inv"][:n])
    for tile in (256, 512, 0):
        fresh_gpu.set_fr_scan_tile(tile)
        assert gpu_product(fresh_gpu, data["num_b"], data["den_b"],
                           None) == want, f"tile {tile}"
        assert gpu_invert(fresh_gpu, data["den_b"]) == want_inv, f"tile {tile}"


def test_zero_denominator(fresh_gpu, data):
    for tile in (256, 0):
        fresh_gpu.set_fr_scan_tile(tile)
        T = tile_in_force(tile)
        n = 3 * T + 5
        for j in (0, T - 1, T + 7, n - 1):
            den = list(data["den"][:n])
            den[j] = 0
            z, last = gpu_product(fresh_gpu, data["num_b"][:32 * n],
                                  mont(den), data["z0"])
            want_z, _ = want_product(data, n, True, data["z0"])
            assert z[:32 * (j + 1)] == want_z[:32 * (j + 1)], f"j={j} head"
            assert z[32 * (j + 1):] == ZERO * (n - j - 1), f"j={j} tail"
            assert last == ZERO, f"j={j} out_last"


def test_aliasing(fresh_gpu, data):
    for tile in (256, 0):
        fresh_gpu.set_fr_scan_tile(tile)
        n = 3 * tile_in_force(tile) + 5
        num_b, den_b = data["num_b"][:32 * n], data["den_b"][:32 * n]
        want = want_product(data, n, True, data["z0"])
        assert gpu_product(fresh_gpu, num_b, den_b, data["z0"], "num") == want
        assert gpu_product(fresh_gpu, num_b, den_b, data["z0"], "den") == want
        assert gpu_product(fresh_gpu, num_b, None, None, "num") == \
            want_product(data, n, False, None)


def test_chaining(fresh_gpu, data):
    """Two calls on the halves of a vector, the second seeded with the
    first's out_last, equal one call on the whole vector."""
    n, h = 2 * 1024 + 77, 1024 + 13
    num_b, den_b = data["num_b"][:32 * n], data["den_b"][:32 * n]
    z, last = gpu_product(fresh_gpu, num_b, den_b, data["z0"])
    za, la = gpu_product(fresh_gpu, num_b[:32 * h], den_b[:32 * h], data["z0"])
    zb, lb = gpu_product(fresh_gpu, num_b[32 * h:], den_b[32 * h:],
                         ref.from_mont_bytes(la, R))
    assert za + zb == z
    assert lb == last
    assert (z, last) == want_product(data, n, True, data["z0"])


def test_pipeline_product_intt_commit(fresh_gpu, oracle, data):
    """grand product -> inverse NTT -> MSM, all on device buffers, equals the
    same chain started from the host-computed Z uploaded."""
    g = fresh_gpu
    log_n = 12
    n = 1 << log_n
    _, bases = oracle.gen_msm_inputs(n, seed=4104, fast=True)
    w = ref.fr_root_of_unity(log_n)
    w_inv = ref.to_mont_bytes(pow(w, -1, R), R)
    want_z, _ = want_product(data, n, True, None)
    d = Dev(g)
    d_bases = d.put(bases)
    d_num = d.put(data["num_b"][:32 * n])
    d_den = d.put(data["den_b"][:32 * n])
    d_z = d.put(b"\xa5" * (32 * n))
    d_host = d.put(want_z)
    g.fr_grand_product(d_num, d_den, None, d_z, n)
    results = []
    for buf in (d_z, d_host):
        g.ntt_device(buf, log_n, w_inv, inverse=True)
        results.append((d.get(buf, n),
                        g.msm_device(d_bases, buf, n, canonical=False)))
    d.free()
    assert results[0][0] == results[1][0], "coefficients differ"
    assert results[0][1] == results[1][1], "commitments differ"
    assert results[0][1] != bytes(64)


def test_error_paths(fresh_gpu, data):
    g = fresh_gpu
    n = 300
    d = Dev(g)
    d_a = d.put(data["num_b"][:32 * n])
    d_b = d.put(data["den_b"][:32 * n])
    too_many = (1 << 28) + 1
    with pytest.raises(RuntimeError, match="2\\^28"):
        g.fr_batch_invert(d_a, d_b, too_many)
    with pytest.raises(RuntimeError, match="2\\^28"):
        g.fr_grand_product(d_a, d_b, None, d_b, too_many)
    with pytest.raises(RuntimeError, match="null"):
        g.fr_batch_invert(0, d_b, n)
    with pytest.raises(RuntimeError, match="null"):
        g.fr_batch_invert(d_a, 0, n)
    with pytest.raises(RuntimeError, match="null"):
        g.fr_grand_product(0, d_b, None, d_b, n)
    with pytest.raises(RuntimeError, match="null"):
        g.fr_grand_product(d_a, d_b, None, 0, n)
    with pytest.raises(RuntimeError, match="invalid ctx/device"):
        g.fr_batch_invert(d_a, d_b, n, dev=7)
    g.set_fr_scan_tile(512)
    for bad in (100, 257, 2 * tile_in_force(0)):
        with pytest.raises(RuntimeError, match="set_fr_scan_tile"):
            g.set_fr_scan_tile(bad)
    # the setting survived the rejected values, and valid calls still work
    g.fr_batch_invert(d_b, d_b, n)
    assert d.get(d_b, n) == mont(data["den_inv"][:n])
    g.upload(d_b, data["den_b"][:32 * n])
    last = g.fr_grand_product(d_a, d_b, None, d_b, n)
    want_z, want_last = want_product(data, n, True, None)
    assert d.get(d_b, n) == want_z
    assert last == want_last
    d.free()
