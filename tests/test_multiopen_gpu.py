"""GPU checks of spectre_gpu_fr_lincomb, spectre_gpu_fr_poly_eval_batch and
spectre_gpu_fr_poly_div_roots.

The reference is plain Python integers (tests/multiopen_ref.py over
tests/golden/bn254_ref.py, loaded by path), and every result is also compared
with the existing single calls it stands for: the fr_vec_op SCALE /
ADD_SCALED chain, fr_poly_eval per polynomial, fr_poly_div_linear per root.
Every comparison is byte-exact; there is no tolerance anywhere. The module's
polynomials are generated once and sliced per case. Output buffers carry a
sentinel element behind the last one. A test that changes the tile owns its
context and restores the default before closing it."""
import ctypes
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "multiopen_ref", os.path.join(HERE, "multiopen_ref.py"))
mr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mr)
R, enc, mont, ints = mr.R, mr.enc, mr.mont, mr.ints

N_LEVELS = 256 * 256 + 1    # tile 256: 65 537 -> 257 -> 2 -> 1
N_MAX = N_LEVELS + 300      # the tile-independence size
N_SMALL = 1029
N_BIG = 5                   # polynomials of N_MAX coefficients
N_POOL = 32                 # polynomials of N_SMALL coefficients
FILL = b"\xa5" * 32


@pytest.fixture(scope="module")
def data(oracle):
    """big: N_BIG polynomials of N_MAX coefficients; small: N_POOL of
    N_SMALL; every one as bytes and as integers, pairwise different, with 0
    and R - 1 among the elements. rnd: field elements for points, roots,
    coefficients and challenges."""
    def split(raw, count, n):
        polys = []
        for k in range(count):
            b = bytearray(raw[32 * n * k:32 * n * (k + 1)])
            # 0 and R - 1 at rows every tested size keeps (n >= 1: row 0)
            b[0:32] = enc(0) if k % 2 == 0 else enc(R - 1)
            if n > 200:
                b[32 * 200:32 * 201] = enc(R - 1) if k % 2 == 0 else enc(0)
            polys.append(bytes(b))
        return polys
    big_b = split(oracle.gen_fr_vector(N_BIG * N_MAX, seed=6101), N_BIG, N_MAX)
    small_b = split(oracle.gen_fr_vector(N_POOL * N_SMALL, seed=6102),
                    N_POOL, N_SMALL)
    return {"big_b": big_b, "big": [ints(b) for b in big_b],
            "small_b": small_b, "small": [ints(b) for b in small_b],
            "rnd": ints(oracle.gen_fr_vector(64, seed=6103))}


@pytest.fixture
def fresh_gpu():
    from spectre_amd import SpectreGpu
    g = SpectreGpu([0])
    yield g
    g.set_fr_scan_tile(0)
    g.close()


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

    def out(self, n: int) -> int:
        """n + 1 sentinel elements: n of output and one that must stay."""
        return self.put(FILL * (n + 1))

    def get(self, p: int, n: int) -> bytes:
        return self.g.download(p, 32 * n) if n else b""

    def take(self, p: int, n: int) -> bytes:
        """The n output elements of an out() buffer; checks the sentinel."""
        raw = self.g.download(p, 32 * (n + 1))
        assert raw[32 * n:] == FILL, "wrote past n"
        return raw[:32 * n]

    def free(self):
        for p in self.ptrs:
            self.g.free(p)
        self.ptrs = []


# ------------------------------------------------------------------ lincomb
def vec_op_chain(g, d_polys, coeffs, d_out, n):
    """The calls fr_lincomb replaces: one SCALE and m - 1 ADD_SCALED."""
    g.fr_vec_op(g.VEC_SCALE, d_polys[0], None, enc(coeffs[0]), d_out, n)
    for d_p, c in zip(d_polys[1:], coeffs[1:]):
        g.fr_vec_op(g.VEC_ADD_SCALED, d_out, d_p, enc(c), d_out, n)


def lincomb_coeffs(data, m):
    """0, 1 and R - 1 beside random ones, as far as m allows."""
    rnd = data["rnd"]
    small = {1: [rnd[0]], 2: [R - 1, rnd[1]], 3: [1, rnd[2], 0]}
    return small[m] if m <= 3 else [0, 1, R - 1] + rnd[3:m]


LINCOMB_SHAPES = [(3, n) for n in (0, 1, 255, 256, 257, 1029)] + \
    [(m, 257) for m in (1, 2, 31, 32)]


@pytest.mark.parametrize("m,n", LINCOMB_SHAPES)
def test_lincomb(gpu, data, m, n):
    coeffs = lincomb_coeffs(data, m)
    polys_b = [b[:32 * n] for b in data["small_b"][:m]]
    polys = [p[:n] for p in data["small"][:m]]
    d = Dev(gpu)
    d_polys = [d.put(b) for b in polys_b]
    d_out, d_chain = d.out(n), d.out(n)
    gpu.fr_lincomb(d_polys, [enc(c) for c in coeffs], d_out, n)
    got = d.take(d_out, n)
    if n:
        vec_op_chain(gpu, d_polys, coeffs, d_chain, n)
    chain = d.take(d_chain, n)
    for d_p, b in zip(d_polys, polys_b):
        assert d.get(d_p, n) == b, "lincomb wrote an input"
    d.free()
    assert got == mont(mr.lincomb(polys, coeffs, n))
    assert got == chain


def test_lincomb_special_coefficients(gpu, data):
    """All-zero, all-one and all-(R - 1) coefficient lists."""
    n, m = 257, 4
    polys_b = [b[:32 * n] for b in data["small_b"][:m]]
    polys = [p[:n] for p in data["small"][:m]]
    d = Dev(gpu)
    d_polys = [d.put(b) for b in polys_b]
    for c in (0, 1, R - 1):
        d_out = d.out(n)
        gpu.fr_lincomb(d_polys, [enc(c)] * m, d_out, n)
        assert d.take(d_out, n) == mont(mr.lincomb(polys, [c] * m, n)), c
    d.free()


def test_lincomb_aliasing(gpu, data):
    n, m = 1029, 4
    coeffs = data["rnd"][4:4 + m]
    polys_b = [b[:32 * n] for b in data["small_b"][:m]]
    polys = [p[:n] for p in data["small"][:m]]
    cb = [enc(c) for c in coeffs]
    want = mont(mr.lincomb(polys, coeffs, n))
    for where in (0, m - 1):  # d_out is the first / the last input
        d = Dev(gpu)
        d_polys = [d.put(b + FILL) for b in polys_b]
        gpu.fr_lincomb(d_polys, cb, d_polys[where], n)
        assert d.take(d_polys[where], n) == want, f"d_out = input {where}"
        for k in range(m):
            if k != where:
                assert d.take(d_polys[k], n) == polys_b[k]
        d.free()
    d = Dev(gpu)
    d_polys = [d.put(b) for b in polys_b]
    # one pointer listed twice; the accumulator with coefficient one chains
    d_out = d.out(n)
    twice = [d_polys[0], d_polys[1], d_polys[0], d_polys[2]]
    gpu.fr_lincomb(twice, cb, d_out, n)
    assert d.take(d_out, n) == mont(mr.lincomb(
        [polys[0], polys[1], polys[0], polys[2]], coeffs, n))
    gpu.fr_lincomb(d_polys[:2], cb[:2], d_out, n)
    gpu.fr_lincomb([d_out] + d_polys[2:], [enc(1)] + cb[2:], d_out, n)
    assert d.take(d_out, n) == want, "chained through the accumulator"
    # all four inputs one pointer, which is the output too
    d_one = d.put(polys_b[3] + FILL)
    gpu.fr_lincomb([d_one] * m, cb, d_one, n)
    assert d.take(d_one, n) == mont(
        [sum(coeffs) * v % R for v in polys[3]])
    d.free()


def test_lincomb_rejected(gpu, data):
    n = 257
    polys_b = [b[:32 * (n + 2)] for b in data["small_b"][:3]]
    cb = [enc(c) for c in data["rnd"][:33]]
    d = Dev(gpu)
    d_polys = [d.put(b) for b in polys_b]
    d_out = d.out(n)
    with pytest.raises(RuntimeError, match="rc=-.*m 0 outside"):
        gpu.fr_lincomb([], [], d_out, n)
    with pytest.raises(RuntimeError, match="rc=-.*m 33 outside"):
        gpu.fr_lincomb([d_polys[k % 3] for k in range(33)], cb, d_out, n)
    with pytest.raises(RuntimeError, match="rc=-.*null device pointer"):
        gpu.fr_lincomb([d_polys[0], 0, d_polys[2]], cb[:3], d_out, n)
    with pytest.raises(RuntimeError, match="rc=-.*null device pointer"):
        gpu.fr_lincomb(d_polys, cb[:3], 0, n)
    # d_out one element into an input
    with pytest.raises(RuntimeError, match="rc=-.*overlaps"):
        gpu.fr_lincomb(d_polys, cb[:3], d_polys[1] + 32, n)
    with pytest.raises(RuntimeError, match="rc=-.*2\\^28"):
        gpu.fr_lincomb(d_polys, cb[:3], d_out, (1 << 28) + 1)
    with pytest.raises(RuntimeError, match="invalid ctx/device"):
        gpu.fr_lincomb(d_polys, cb[:3], d_out, n, dev=7)
    assert gpu._lib.spectre_gpu_fr_lincomb(
        gpu._ctx, 0, (ctypes.c_void_p * 3)(*d_polys), None, 3,
        ctypes.c_void_p(d_out), n) < 0
    assert b"null" in gpu._lib.spectre_gpu_last_error()
    # nothing was written by the rejected calls
    assert d.get(d_out, n + 1) == FILL * (n + 1)
    for d_p, b in zip(d_polys, polys_b):
        assert d.get(d_p, n + 2) == b
    d.free()


# --------------------------------------------------------------- eval_batch
def eval_points(data, npts):
    return ([0, 1, R - 1] + data["rnd"][8:13])[:npts] if npts >= 3 else \
        data["rnd"][8:8 + npts]


def check_eval_batch(g, polys_b, polys, n, pts, single=True):
    d = Dev(g)
    d_polys = [d.put(b[:32 * n]) for b in polys_b]
    pb = [enc(x) for x in pts]
    got = g.fr_poly_eval_batch(d_polys, n, pb)
    per_poly = [g.fr_poly_eval(d_p, n, pb) for d_p in d_polys] if single \
        else got
    for d_p, b in zip(d_polys, polys_b):
        assert d.get(d_p, n) == b[:32 * n], "eval_batch wrote an input"
    d.free()
    assert got == [[enc(mr.horner(a[:n], x)) for x in pts] for a in polys]
    assert got == per_poly
    return got


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, N_LEVELS])
def test_eval_batch_5x3(fresh_gpu, data, n):
    """m != npoints, different polynomials, different points: a swapped k / p
    index cannot pass. n = 65 537 runs three levels at tile 256."""
    fresh_gpu.set_fr_scan_tile(256)
    check_eval_batch(fresh_gpu, data["big_b"], data["big"], n,
                     eval_points(data, 3))


@pytest.mark.parametrize("m,npts,n", [(32, 8, 257), (2, 2, N_LEVELS),
                                      (1, 1, 257), (1, 1, 1)])
def test_eval_batch_shapes(fresh_gpu, data, m, npts, n):
    """(32, 8): the largest vector count and readback; (2, 2) at 65 537:
    three levels; (1, 1): the single call's shape through the table."""
    fresh_gpu.set_fr_scan_tile(256)
    pool = "big" if n > N_SMALL else "small"
    check_eval_batch(fresh_gpu, data[pool + "_b"][:m], data[pool][:m], n,
                     eval_points(data, npts))


def test_eval_batch_default_tile(gpu, data):
    check_eval_batch(gpu, data["small_b"][:5], data["small"][:5], N_SMALL,
                     eval_points(data, 3))


def test_eval_batch_pointer_twice(fresh_gpu, data):
    fresh_gpu.set_fr_scan_tile(256)
    order = [0, 1, 0, 2, 2]
    check_eval_batch(fresh_gpu, [data["small_b"][k] for k in order],
                     [data["small"][k] for k in order], 257,
                     eval_points(data, 3))
    g, n = fresh_gpu, 257
    d = Dev(g)
    d_a = d.put(data["small_b"][0][:32 * n])
    pb = [enc(x) for x in eval_points(data, 2)]
    got = g.fr_poly_eval_batch([d_a, d_a], n, pb)
    d.free()
    assert got[0] == got[1]
    assert got[0] == [enc(mr.horner(data["small"][0][:n], x))
                      for x in eval_points(data, 2)]


def test_eval_batch_tile_independence(fresh_gpu, data):
    g, n = fresh_gpu, N_MAX
    pts = data["rnd"][13:16]
    want = [[enc(mr.horner(a, x)) for x in pts] for a in data["big"][:2]]
    d = Dev(g)
    d_polys = [d.put(b) for b in data["big_b"][:2]]
    for tile in (0, 256):
        g.set_fr_scan_tile(tile)
        got = g.fr_poly_eval_batch(d_polys, n, [enc(x) for x in pts])
        assert got == want, f"tile {tile}"
    d.free()


def test_eval_batch_rejected(gpu, data):
    n = 257
    d = Dev(gpu)
    d_polys = [d.put(b[:32 * n]) for b in data["small_b"][:3]]
    pb = [enc(x) for x in data["rnd"][:9]]
    with pytest.raises(RuntimeError, match="rc=-.*m 0 outside"):
        gpu.fr_poly_eval_batch([], n, pb[:2])
    with pytest.raises(RuntimeError, match="rc=-.*m 33 outside"):
        gpu.fr_poly_eval_batch([d_polys[k % 3] for k in range(33)], n, pb[:2])
    with pytest.raises(RuntimeError, match="rc=-.*npoints 0 outside"):
        gpu.fr_poly_eval_batch(d_polys, n, [])
    with pytest.raises(RuntimeError, match="rc=-.*npoints 9 outside"):
        gpu.fr_poly_eval_batch(d_polys, n, pb)
    with pytest.raises(RuntimeError, match="rc=-.*null device pointer"):
        gpu.fr_poly_eval_batch([d_polys[0], 0], n, pb[:2])
    with pytest.raises(RuntimeError, match="rc=-.*2\\^28"):
        gpu.fr_poly_eval_batch(d_polys, (1 << 28) + 1, pb[:2])
    # a rejected call leaves the host output alone
    out = (ctypes.c_uint8 * (32 * 6)).from_buffer_copy(FILL * 6)
    pts = (ctypes.c_uint8 * 64).from_buffer_copy(pb[0] + pb[1])
    assert gpu._lib.spectre_gpu_fr_poly_eval_batch(
        gpu._ctx, 0, (ctypes.c_void_p * 3)(*d_polys), 3, n, pts, 9, out) < 0
    assert bytes(out) == FILL * 6
    # and a valid call still works
    got = gpu.fr_poly_eval_batch(d_polys, n, pb[:2])
    assert got[2][1] == enc(mr.horner(data["small"][2][:n], data["rnd"][1]))
    d.free()


# ---------------------------------------------------------------- div_roots
def div_root_list(data, nroots):
    z = data["rnd"][16:19]
    return [z[0], z[0], 0, 1, z[1], R - 1, z[1], z[2]][:nroots]


def gpu_div_roots(g, a_b, roots, in_place=False, want_rems=True):
    n = len(a_b) // 32
    d = Dev(g)
    d_a = d.put(a_b + FILL)
    d_q = d_a if in_place else d.out(n)
    rems = g.fr_poly_div_roots(d_a, [enc(z) for z in roots], d_q, n,
                               want_rems=want_rems)
    q = d.take(d_q, n)
    if not in_place:
        assert d.take(d_a, n) == a_b, "div_roots wrote its input"
    d.free()
    return q, rems


def gpu_div_chain(g, a_b, roots):
    """The calls fr_poly_div_roots replaces."""
    n = len(a_b) // 32
    d = Dev(g)
    d_a = d.put(a_b)
    d_q = d.out(n)
    rems = []
    for j, z in enumerate(roots):
        rems.append(g.fr_poly_div_linear(d_a if j == 0 else d_q, enc(z), d_q,
                                         n))
    q = d.take(d_q, n)
    d.free()
    return q, rems


def check_div_roots(g, a_b, a, roots):
    n = len(a)
    want_q, want_rems = mr.div_roots(a, roots)
    want = (mont(want_q), [enc(r) for r in want_rems])
    out_of_place = gpu_div_roots(g, a_b, roots)
    assert out_of_place[0] == want[0], "quotient"
    assert out_of_place[1] == want[1], "remainders"
    assert gpu_div_roots(g, a_b, roots, in_place=True) == want
    assert gpu_div_chain(g, a_b, roots) == want
    assert gpu_div_roots(g, a_b, roots, want_rems=False) == (want[0], None)
    top = min(len(roots), n)
    assert want[0][32 * (n - top):] == bytes(32 * top)


@pytest.mark.parametrize("nroots", [1, 2, 3, 8])
def test_div_roots(fresh_gpu, data, nroots):
    """n in {0, 1, 2, 9, 257}, n < nroots among them; the roots hold a
    repeated one from 2 on, 0 from 3 on, 1 and R - 1 at 8."""
    fresh_gpu.set_fr_scan_tile(256)
    roots = div_root_list(data, nroots)
    for n in (0, 1, 2, 9, 257):
        check_div_roots(fresh_gpu, data["small_b"][1][:32 * n],
                        data["small"][1][:n], roots)


def test_div_roots_zero_one_and_small(fresh_gpu, data):
    fresh_gpu.set_fr_scan_tile(256)
    for roots in ([0], [1], [0, 1, data["rnd"][19]]):
        for n in (2, 257):
            check_div_roots(fresh_gpu, data["small_b"][2][:32 * n],
                            data["small"][2][:n], roots)


def test_div_roots_three_levels(fresh_gpu, data):
    fresh_gpu.set_fr_scan_tile(256)
    n = N_LEVELS
    check_div_roots(fresh_gpu, data["big_b"][0][:32 * n], data["big"][0][:n],
                    data["rnd"][20:22])


def test_div_roots_default_tile(gpu, data):
    check_div_roots(gpu, data["small_b"][3], data["small"][3],
                    div_root_list(data, 4))


def test_div_roots_exact_product(fresh_gpu, data):
    """a = Z_S q0 built in integers: every remainder is zero and q == q0."""
    fresh_gpu.set_fr_scan_tile(256)
    roots = [data["rnd"][22], 0, 1, data["rnd"][22]]
    q0 = data["small"][4][:600]
    a = mr.poly_mul(mr.vanishing(roots), q0)
    q, rems = gpu_div_roots(fresh_gpu, mont(a), roots)
    assert rems == [bytes(32)] * 4
    assert q == data["small_b"][4][:32 * 600] + bytes(32 * 4)


def test_div_roots_rejected(gpu, data):
    n = 257
    a_b = data["small_b"][0][:32 * (n + 2)]
    zb = [enc(z) for z in data["rnd"][:9]]
    d = Dev(gpu)
    d_a = d.put(a_b)
    d_q = d.out(n)
    with pytest.raises(RuntimeError, match="rc=-.*nroots 0 outside"):
        gpu.fr_poly_div_roots(d_a, [], d_q, n)
    with pytest.raises(RuntimeError, match="rc=-.*nroots 9 outside"):
        gpu.fr_poly_div_roots(d_a, zb, d_q, n)
    with pytest.raises(RuntimeError, match="rc=-.*null"):
        gpu.fr_poly_div_roots(0, zb[:2], d_q, n)
    with pytest.raises(RuntimeError, match="rc=-.*null"):
        gpu.fr_poly_div_roots(d_a, zb[:2], 0, n)
    with pytest.raises(RuntimeError, match="rc=-.*overlaps"):
        gpu.fr_poly_div_roots(d_a, zb[:2], d_a + 32, n)
    with pytest.raises(RuntimeError, match="rc=-.*2\\^28"):
        gpu.fr_poly_div_roots(d_a, zb[:2], d_q, (1 << 28) + 1)
    assert d.get(d_q, n + 1) == FILL * (n + 1)
    assert d.get(d_a, n + 2) == a_b
    d.free()


# ------------------------------------------------ one opening, on the device
def test_two_set_opening_closes_on_the_device(gpu, data):
    """S_1 = {x} with three polynomials, S_2 = {x, wx, w^2 x} with two, n =
    2^11, every vector step on the device: eval_batch per set, f_i by
    lincomb, n_i and the Newton form of r_i by div_roots with nothing
    subtracted first, h by lincomb, L by ONE lincomb and a 32-byte fix of
    coefficient 0, W by fr_poly_div_linear at u. The remainder of the last
    division is zero and h and W equal the integer computation byte for byte.

    This pins the algebra. The order in which PSE's SHPLONK draws and applies
    y, v and u is an [assump] of CALLCOUNTS.md, as for the other stages; the
    integers here follow tests/multiopen_ref.py::shplonk_open."""
    g = gpu
    log_n = 11
    n = 1 << log_n
    w = mr.ref.fr_root_of_unity(log_n)
    x, y, v, u = data["rnd"][24:28]
    sets = [([x], list(range(0, 3))),
            ([x, w * x % R, w * w * x % R], list(range(3, 5)))]
    polys = [p[:n] for p in data["big"]]
    want = mr.shplonk_open([(pts, [polys[k] for k in ks])
                            for pts, ks in sets], y, v, u, n)
    d = Dev(g)
    d_p = [d.put(b[:32 * n]) for b in data["big_b"]]
    d_f, d_n, rems = [], [], []
    for i, (pts, ks) in enumerate(sets):
        # 1. the set's evaluations
        evals = g.fr_poly_eval_batch([d_p[k] for k in ks], n,
                                     [enc(z) for z in pts])
        # 2. f_i = sum_k y^k p_{i,k}
        d_f.append(d.out(n))
        g.fr_lincomb([d_p[k] for k in ks],
                     [enc(pow(y, k, R)) for k in range(len(ks))], d_f[i], n)
        assert d.take(d_f[i], n) == mont(want["f"][i])
        # 3. n_i and r_i; r_i is the interpolant of the combined evaluations
        d_n.append(d.out(n))
        rems.append(g.fr_poly_div_roots(d_f[i], [enc(z) for z in pts],
                                        d_n[i], n))
        comb = [sum(pow(y, k, R) * ints(evals[k][p])[0]
                    for k in range(len(ks))) % R for p in range(len(pts))]
        assert rems[i] == [enc(c) for c in mr.newton_from_evals(pts, comb)]
        assert rems[i] == [enc(r) for r in want["rems"][i]]
    # 4. h = sum_i v^i n_i
    d_h = d.out(n)
    g.fr_lincomb(d_n, [enc(pow(v, i, R)) for i in range(2)], d_h, n)
    assert d.take(d_h, n) == mont(want["h"])
    # 5. L, from scalars the caller computes on the host
    r_u = [mr.horner(mr.newton(ints(b"".join(rems[i])), sets[i][0]), u)
           for i in range(2)]
    coeffs = [pow(v, i, R) * want["zdiff"][i] % R for i in range(2)]
    d_l = d.out(n)
    g.fr_lincomb(d_f + [d_h], [enc(c) for c in coeffs] + [enc(-want["z_t"])],
                 d_l, n)
    l0 = ints(g.download(d_l, 32))[0]
    g.upload(d_l, enc(l0 - sum(c * r for c, r in zip(coeffs, r_u))))
    # 6. W = L / (X - u)
    d_w = d.out(n)
    rem = g.fr_poly_div_linear(d_l, enc(u), d_w, n)
    got_w = d.take(d_w, n)
    d.free()
    # 7.
    assert rem == bytes(32)
    assert got_w == mont(want["W"])
