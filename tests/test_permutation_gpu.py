"""GPU checks of spectre_gpu_fr_powers / spectre_gpu_fr_permutation_terms.

The reference is tests/permutation_ref.py (plain Python integers, loaded by
path); every comparison is byte-exact. Outputs are poisoned with 0xa5 and one
element longer than the call writes; that element must come back untouched.
Columns, challenges and the valid permutations are computed once per module
and left unchanged."""
import importlib.util
import os
import random

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


pr = _load("permutation_ref")
edge = _load("edge_operands")
R, DELTA = pr.R, pr.DELTA
root = pr.ref.fr_root_of_unity
POISON = b"\xa5" * 32
ONE = pr.enc(1)

T1 = 4096  # low-table entries: g^i = T1[i & 0xfff] * T2[i >> 12]
POWER_SIZES = [1, 2, 255, 256, 257, T1 - 1, T1, T1 + 1, 2 * T1 + 5]
TERM_COLS = [1, 2, 3, 8]
TERM_SIZES = [1, 257, T1 + 1, 3 * T1 + 5]
N_MAX = max(TERM_SIZES)


def log2_ceil(n: int) -> int:
    return max(1, (n - 1).bit_length())


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
        """n elements and a guard, all poisoned."""
        return self.put(POISON * (n + 1))

    def get(self, p: int, n: int) -> bytes:
        return self.g.download(p, 32 * n) if n else b""

    def get_guarded(self, p: int, n: int, what: str) -> bytes:
        data = self.g.download(p, 32 * (n + 1))
        assert data[32 * n:] == POISON, f"{what}: wrote past element {n}"
        return data[:32 * n]

    def free(self):
        for p in self.ptrs:
            self.g.free(p)
        self.ptrs = []


@pytest.fixture
def dev(gpu):
    d = Dev(gpu)
    yield d
    d.free()


# ------------------------------------------------------------------ fr_powers
def gpu_powers(d, c, g, n):
    p = d.out(n)
    d.g.fr_powers(None if c is None else pr.enc(c), pr.enc(g), p, n)
    return d.get_guarded(p, n, "fr_powers")


@pytest.mark.parametrize("n", POWER_SIZES)
def test_powers_against_python(dev, n):
    rng = random.Random(0x70e5 + n)
    g_rand, c_rand = rng.randrange(2, R), rng.randrange(1, R)
    cases = [("random g, random c", c_rand, g_rand),
             ("random g, c NULL", None, g_rand),
             ("g = 1", c_rand, 1),
             ("g = 0", c_rand, 0),
             ("g = 0, c NULL", None, 0),
             ("g the 2^k root", None, root(log2_ceil(n))),
             ("g the 2^k root, random c", c_rand, root(log2_ceil(n)))]
    for what, c, g in cases:
        got = gpu_powers(dev, c, g, n)
        assert got == pr.mont(pr.powers(1 if c is None else c, g, n)), \
            f"n={n}: {what}"


def test_powers_equal_the_ntt_of_the_unit_vector(dev, gpu):
    """2^18 rows, g = omega: all 64 high-table entries, checked against the
    oracle-pinned transform of e_1, which is omega^t."""
    log_n = 18
    n = 1 << log_n
    w = pr.enc(root(log_n))
    d_e1 = dev.put(bytes(32) + ONE + bytes(32 * (n - 2)))
    gpu.ntt_device(d_e1, log_n, w)
    want = dev.get(d_e1, n)
    d_out = dev.out(n)
    gpu.fr_powers(None, w, d_out, n)
    got = dev.get_guarded(d_out, n, "fr_powers")
    assert got[:64] == ONE + w
    assert got == want


# ------------------------------------------------------- fr_permutation_terms
@pytest.fixture(scope="module")
def columns():
    """8 value and 8 sigma columns of N_MAX canonical values: random, with
    the edge images of tests/edge_operands.py (0, 1, r - 1, 2^253, the
    all-ones-low image, ...) and the images around 2^255 - r in their first
    rows, every image against every column by a per-column rotation."""
    rng = random.Random(0x9e2a)
    imgs = list(edge.specials(R))
    imgs += [x % R for x in ((1 << 255) - R - 1, (1 << 255) - R,
                             (1 << 255) - R + 1, (1 << 256) - 2 * R)]
    assert {0, 1, R - 1} <= set(imgs)
    canon = [x * pr.MONT_INV % R for x in imgs]
    cols = []
    for k in range(16):
        col = [rng.randrange(R) for _ in range(N_MAX)]
        for t in range(len(canon)):
            # rows past a small n simply fall away; n = 1 sees row 0
            col[t] = canon[(t + 5 * k) % len(canon)]
        cols.append(col)
    return {"values": cols[:8], "sigmas": cols[8:],
            "beta": rng.randrange(1, R), "gamma": rng.randrange(1, R),
            "omega_free": rng.randrange(2, R)}


def planted(columns, m, n, omega, delta0):
    """The first m columns cut to n rows, with one row whose denominator is
    exactly zero and one whose numerator is. Returns (values, sigmas,
    den_row, num_row); num_row is None where it would need the cell the
    denominator row already took (m = 1, n = 1)."""
    beta, gamma = columns["beta"], columns["gamma"]
    values = [list(c[:n]) for c in columns["values"][:m]]
    sigmas = [c[:n] for c in columns["sigmas"][:m]]
    den_row, num_row = n // 3, (2 * n) // 3
    values[0][den_row] = -(beta * sigmas[0][den_row] + gamma) % R
    if (den_row, 0) == (num_row, m - 1):
        return values, sigmas, den_row, None
    j = m - 1
    values[j][num_row] = -(beta * delta0 * pow(DELTA, j, R)
                           * pow(omega, num_row, R) + gamma) % R
    return values, sigmas, den_row, num_row


@pytest.mark.parametrize("n", TERM_SIZES)
@pytest.mark.parametrize("m", TERM_COLS)
def test_terms_against_python(dev, gpu, columns, m, n):
    beta, gamma = columns["beta"], columns["gamma"]
    seen_num_zero = False
    for delta0 in (None, pow(DELTA, 5, R)):
        for omega in (root(log2_ceil(n)), columns["omega_free"]):
            what = f"m={m} n={n} delta0={delta0 is not None} omega={omega:#x}"
            d0 = 1 if delta0 is None else delta0
            values, sigmas, den_row, num_row = planted(columns, m, n, omega, d0)
            want_num, want_den = pr.terms(values, sigmas, beta, gamma, omega,
                                          d0, DELTA, n)
            assert want_den[den_row] == 0, what
            if num_row is not None:
                assert want_num[num_row] == 0, what
                seen_num_zero = True
            in_b = [pr.mont(c) for c in values + sigmas]
            d_in = [dev.put(b) for b in in_b]
            d_num, d_den = dev.out(n), dev.out(n)
            gpu.fr_permutation_terms(
                d_in[:m], d_in[m:], pr.enc(beta), pr.enc(gamma), pr.enc(omega),
                None if delta0 is None else pr.enc(delta0), pr.enc(DELTA),
                d_num, d_den, n)
            got_num = dev.get_guarded(d_num, n, "d_num")
            got_den = dev.get_guarded(d_den, n, "d_den")
            assert got_den == pr.mont(want_den), what
            assert got_num == pr.mont(want_num), what
            assert got_den[32 * den_row:32 * den_row + 32] == bytes(32)
            for p, b in zip(d_in, in_b):
                assert dev.get(p, n) == b, f"{what}: an input was written"
            dev.free()
    assert seen_num_zero or (m, n) == (1, 1)


# ------------------------------------------------------------ chain on device
def device_chain(d, values, sigmas, chunk, beta, gamma, omega, n, u):
    """terms -> fr_grand_product per chunk, as a caller chains them. Returns
    [(z bytes over u rows, out_last bytes)] and the device Z buffers."""
    g = d.g
    d_vals = [d.put(pr.mont(c)) for c in values]
    d_sigs = [d.put(pr.mont(c)) for c in sigmas]
    d_num, d_den = d.out(n), d.out(n)
    out, bufs = [], []
    last, delta0 = None, None
    for c0 in range(0, len(values), chunk):
        g.fr_permutation_terms(
            d_vals[c0:c0 + chunk], d_sigs[c0:c0 + chunk], pr.enc(beta),
            pr.enc(gamma), pr.enc(omega), delta0, pr.enc(DELTA), d_num, d_den,
            n)
        d_z = d.out(u)
        last = g.fr_grand_product(d_num, d_den, last, d_z, u)
        out.append((d.get_guarded(d_z, u, "d_z"), last))
        bufs.append(d_z)
        m = len(d_vals[c0:c0 + chunk])
        delta0 = pr.enc(pow(DELTA, c0 + m, R))
    return out, bufs, d_vals, d_sigs


@pytest.fixture(scope="module")
def chain_case():
    rng = random.Random(0xc4a1)
    n = (1 << 12) + (1 << 9)
    omega = root(13)  # n distinct row labels
    values, sigmas = pr.valid_permutation(5, n, omega, DELTA, rng)
    return {"n": n, "omega": omega, "values": values, "sigmas": sigmas,
            "beta": rng.randrange(1, R), "gamma": rng.randrange(1, R)}


@pytest.mark.parametrize("blinding", [-1, 5])
def test_chain_on_the_device(dev, chain_case, blinding):
    """5 columns in chunks of 2, 2 and 1 over 2^12 + 2^9 rows, u = n and
    u = n - 6: every Z column and every out_last equal halo2's chunk loop."""
    c = chain_case
    n = c["n"]
    u = n - blinding - 1
    want = pr.commit_chunks(c["values"], c["sigmas"], 2, c["beta"], c["gamma"],
                            c["omega"], DELTA, n, blinding)
    got, _, _, _ = device_chain(dev, c["values"], c["sigmas"], 2, c["beta"],
                                c["gamma"], c["omega"], n, u)
    assert len(got) == len(want) == 3
    for k, ((z, last), (want_z, want_last)) in enumerate(zip(got, want)):
        assert z == pr.mont(want_z), f"chunk {k}: Z column"
        assert last == pr.enc(want_last), f"chunk {k}: out_last"
    if u == n:
        assert got[-1][1] == ONE, "the product over all rows does not close"
    else:
        assert got[-1][1] != ONE


def test_constraint_closes_on_the_device(dev, gpu):
    """The quotient-phase use of the powers column: with Z from the calls
    above and X = fr_powers(NULL, omega, n), one gate_eval program computes
      z(omega X) prod(v_j + beta sigma_j + gamma)
        - z(X) prod(v_j + beta delta^j X + gamma)
    which is zero on every row, the wrap-around row included, because the
    product of a valid permutation closes to 1."""
    rng = random.Random(0xc105e)
    m, log_n = 3, 13
    n = 1 << log_n
    omega = root(log_n)
    values, sigmas = pr.valid_permutation(m, n, omega, DELTA, rng)
    beta, gamma = rng.randrange(1, R), rng.randrange(1, R)
    ((_, last),), (d_z,), d_vals, d_sigs = device_chain(
        dev, values, sigmas, m, beta, gamma, omega, n, n)
    assert last == ONE
    d_x = dev.out(n)
    gpu.fr_powers(None, pr.enc(omega), d_x, n)
    assert dev.get_guarded(d_x, n, "X") == pr.mont(pr.powers(1, omega, n))

    G = gpu
    cols = [d_z, d_x] + d_vals + d_sigs  # z, X, v_0.., sigma_0..
    consts = [beta, gamma] + [beta * pow(DELTA, j, R) % R for j in range(m)]
    prog = [(G.GATE_COL, 0, 1)]                      # z(omega X)
    for j in range(m):
        prog += [(G.GATE_COL, 2 + j, 0), (G.GATE_CONST, 0, 0),
                 (G.GATE_COL, 2 + m + j, 0), (G.GATE_MUL, 0, 0),
                 (G.GATE_ADD, 0, 0), (G.GATE_CONST, 1, 0), (G.GATE_ADD, 0, 0),
                 (G.GATE_MUL, 0, 0)]
    prog += [(G.GATE_COL, 0, 0)]                     # z(X)
    for j in range(m):
        prog += [(G.GATE_CONST, 2 + j, 0), (G.GATE_COL, 1, 0),
                 (G.GATE_MUL, 0, 0), (G.GATE_COL, 2 + j, 0),
                 (G.GATE_ADD, 0, 0), (G.GATE_CONST, 1, 0), (G.GATE_ADD, 0, 0),
                 (G.GATE_MUL, 0, 0)]
    prog += [(G.GATE_SUB, 0, 0)]
    depth = peak = 0
    for op, _, _ in prog:
        depth += 1 if op in (G.GATE_COL, G.GATE_CONST) else -1
        peak = max(peak, depth)
    assert depth == 1 and peak <= 4
    d_res = dev.out(n)
    gpu.gate_eval(cols, pr.mont(consts), prog, n, rot_scale=1, d_out=d_res)
    assert dev.get_guarded(d_res, n, "gate_eval") == bytes(32 * n)
    # the program does tell a broken column from a valid one
    bad = list(values[1])
    bad[n - 1] = (bad[n - 1] + 1) % R
    gpu.upload(d_vals[1], pr.mont(bad))
    gpu.gate_eval(cols, pr.mont(consts), prog, n, rot_scale=1, d_out=d_res)
    res = dev.get(d_res, n)
    assert res[32 * (n - 1):] != bytes(32)
    assert res[:32 * (n - 1)] == bytes(32 * (n - 1))


# ------------------------------------------------- the shared power-table scratch
def test_ntt_and_permutation_calls_share_one_table_buffer(oracle, columns):
    """The coset table of an NTT and the row powers of fr_powers /
    fr_permutation_terms are built into one per-device buffer. One context of
    its own (the buffer starts empty), five calls in a row that grow it, reuse
    it at a smaller n (below 4096, so the low table is short) and switch
    between its users; every result byte-exact."""
    from spectre_amd import SpectreGpu
    rng = random.Random(0x5c7a)
    data = oracle.gen_fr_vector(1 << 13, seed=0x5c7b)
    g5, g5_inv = pr.enc(5), pr.enc(pow(5, -1, R))
    d = Dev(SpectreGpu([0]))
    try:
        def coset_ntt(log_n, inverse):
            src = data[:32 << log_n]
            w = root(log_n)
            w, g = (pow(w, -1, R), g5_inv) if inverse else (w, g5)
            p = d.put(src)
            d.g.ntt_device(p, log_n, pr.enc(w), inverse=inverse, coset_gen=g)
            want = oracle.ntt(src, log_n, pr.enc(w), inverse=inverse,
                              coset_gen=g)
            assert d.get(p, 1 << log_n) == want, \
                f"coset NTT 2^{log_n} inverse={inverse}"

        coset_ntt(13, False)
        n, c, g = 3 * T1 + 5, rng.randrange(1, R), rng.randrange(2, R)
        assert gpu_powers(d, c, g, n) == pr.mont(pr.powers(c, g, n))
        coset_ntt(10, False)
        m, n, omega = 2, 257, root(9)
        beta, gamma = columns["beta"], columns["gamma"]
        values = [c[:n] for c in columns["values"][:m]]
        sigmas = [c[:n] for c in columns["sigmas"][:m]]
        d_in = [d.put(pr.mont(c)) for c in values + sigmas]
        d_num, d_den = d.out(n), d.out(n)
        d.g.fr_permutation_terms(
            d_in[:m], d_in[m:], pr.enc(beta), pr.enc(gamma), pr.enc(omega),
            None, pr.enc(DELTA), d_num, d_den, n)
        want_num, want_den = pr.terms(values, sigmas, beta, gamma, omega, 1,
                                      DELTA, n)
        assert d.get_guarded(d_num, n, "d_num") == pr.mont(want_num)
        assert d.get_guarded(d_den, n, "d_den") == pr.mont(want_den)
        coset_ntt(13, True)
    finally:
        d.free()
        d.g.close()


def test_every_synchronous_call_shares_one_scratch_arena(oracle, columns):
    """All device scratch of the synchronous Fr calls is carved out of one
    per-device arena, and their small readbacks land in one pinned block. One
    context of its own (the arena starts empty, so the growth order is known):
    calls that grow the arena, which moves it, reuse it at a smaller need and
    hand the pinned block from one user to the next. Every result byte-exact
    against the oracle, permutation_ref, lookup_permute_ref or Python
    integers; every guard element untouched."""
    from spectre_amd import SpectreGpu
    lp = _load("lookup_permute_ref")
    rng = random.Random(0xa7e4a)
    data = oracle.gen_fr_vector(1 << 15, seed=0xa7e4b)
    vals = pr.ints(data[:32 * 4100])
    g5 = pr.enc(5)
    d = Dev(SpectreGpu([0]))
    G = d.g
    try:
        def ntt(log_n, coset_gen):
            src, w = data[:32 << log_n], pr.enc(root(log_n))
            p = d.put(src)
            G.ntt_device(p, log_n, w, coset_gen=coset_gen)
            assert d.get(p, 1 << log_n) == oracle.ntt(
                src, log_n, w, coset_gen=coset_gen), f"NTT 2^{log_n}"

        def lookup(a, s):
            u = len(a)
            a_b, s_b = lp.mont(a), lp.mont(s)
            d_a, d_s = d.put(a_b), d.put(s_b)
            d_ap, d_sp = d.out(u), d.out(u)
            try:
                G.fr_lookup_permute(d_a, d_s, d_ap, d_sp, u)
            finally:
                got = (d.get_guarded(d_ap, u, "d_input_perm"),
                       d.get_guarded(d_sp, u, "d_table_perm"))
                assert d.get(d_a, u) == a_b and d.get(d_s, u) == s_b
            return got

        def poly_eval(n, points):
            got = G.fr_poly_eval(d.put(data[:32 * n]), n,
                                 [pr.enc(x) for x in points])
            for x, y in zip(points, got):
                acc = 0
                for c in reversed(vals[:n]):
                    acc = (acc * x + c) % R
                assert y == pr.enc(acc), f"fr_poly_eval n={n} at {x:#x}"

        # 1: tmp and the coset table, two passes
        ntt(13, g5)
        # 2: three tiles of products; the total comes back through the block
        n = 2049
        num, den = vals[:n], vals[n:2 * n]
        z0 = rng.randrange(1, R)
        want_z = [z0]
        for i in range(n):
            want_z.append(want_z[i] * num[i] % R * pr.inv0(den[i]) % R)
        d_z = d.out(n)
        last = G.fr_grand_product(d.put(pr.mont(num)), d.put(pr.mont(den)),
                                  pr.enc(z0), d_z, n)
        assert d.get_guarded(d_z, n, "d_z") == pr.mont(want_z[:n])
        assert last == pr.enc(want_z[n])
        # 3: six extents and hipCUB temp storage: the arena grows and moves
        u = 4097
        table = [vals[rng.randrange(u // 3)] for _ in range(u)]
        inputs = [table[rng.randrange(u)] for _ in range(u)]
        want_a, want_s = lp.serial(inputs, table)
        want_lookup = (lp.mont(want_a), lp.mont(want_s))
        assert lookup(inputs, table) == want_lookup
        # 4: the cached plan's tables are not in the arena and survived
        ntt(13, g5)
        # 5: two levels of partials; evaluations and remainder read back
        n = 1025
        points = [rng.randrange(2, R) for _ in range(3)]
        poly_eval(n, points)
        z = rng.randrange(2, R)
        want_q = [0] * n
        for i in range(n - 2, -1, -1):
            want_q[i] = (vals[i + 1] + z * want_q[i + 1]) % R
        d_q = d.out(n)
        rem = G.fr_poly_div_linear(d.put(data[:32 * n]), pr.enc(z), d_q, n)
        assert d.get_guarded(d_q, n, "d_q") == pr.mont(want_q)
        assert rem == pr.enc((vals[0] + z * want_q[0]) % R)
        # 6: one input value the table does not hold
        absent = vals[u // 3]  # the table draws from the values before it
        assert absent not in table
        with pytest.raises(RuntimeError,
                           match=r"rc=-5: .*lookup miss: 1 distinct input "
                                 r"value absent"):
            lookup(inputs[:-1] + [absent], table)
        # 7: the pinned block goes from the miss count to evaluations
        poly_eval(n, points)
        # 8: the row-power table, twice
        m, n, omega = 2, 4097, root(13)
        beta, gamma = columns["beta"], columns["gamma"]
        values = [c[:n] for c in columns["values"][:m]]
        sigmas = [c[:n] for c in columns["sigmas"][:m]]
        d_in = [d.put(pr.mont(c)) for c in values + sigmas]
        d_num, d_den = d.out(n), d.out(n)
        G.fr_permutation_terms(d_in[:m], d_in[m:], pr.enc(beta),
                               pr.enc(gamma), pr.enc(omega), None,
                               pr.enc(DELTA), d_num, d_den, n)
        want_num, want_den = pr.terms(values, sigmas, beta, gamma, omega, 1,
                                      DELTA, n)
        assert d.get_guarded(d_num, n, "d_num") == pr.mont(want_num)
        assert d.get_guarded(d_den, n, "d_den") == pr.mont(want_den)
        c, g = rng.randrange(1, R), rng.randrange(2, R)
        assert gpu_powers(d, c, g, n) == pr.mont(pr.powers(c, g, n))
        # 9: column pointers, one constant and the program, staged
        n, k = 256, rng.randrange(1, R)
        d_res = d.out(n)
        G.gate_eval([d.put(data[:32 * n]), d.put(data[32 * n:64 * n])],
                    pr.enc(k),
                    [(G.GATE_COL, 0, 0), (G.GATE_COL, 1, 0),
                     (G.GATE_MUL, 0, 0), (G.GATE_CONST, 0, 0),
                     (G.GATE_ADD, 0, 0)], n, rot_scale=1, d_out=d_res)
        assert d.get_guarded(d_res, n, "gate_eval") == pr.mont(
            [(a * b + k) % R for a, b in zip(vals[:n], vals[n:2 * n])])
        # 10: the arena grows again
        ntt(15, None)
        # 11: reuse at a smaller need
        assert lookup(inputs, table) == want_lookup
    finally:
        d.free()
        d.g.close()


# ------------------------------------------------------------ argument checks
def test_argument_checks(dev, gpu, columns):
    n = 300
    beta, gamma = pr.enc(columns["beta"]), pr.enc(columns["gamma"])
    w, dl = pr.enc(root(9)), pr.enc(DELTA)
    in_b = [pr.mont(c[:n]) for c in columns["values"] + columns["sigmas"]]
    d_in = [dev.put(b) for b in in_b]
    d_v, d_s = d_in[:8], d_in[8:]
    d_num, d_den = dev.out(n), dev.out(n)
    too_many = (1 << 28) + 1

    def terms(vals, sigs, num, den, rows):
        gpu.fr_permutation_terms(vals, sigs, beta, gamma, w, None, dl, num,
                                 den, rows)

    with pytest.raises(RuntimeError, match=r"rc=-3.*m 0 outside"):
        terms([], [], d_num, d_den, n)
    with pytest.raises(RuntimeError, match=r"rc=-3.*m 9 outside"):
        terms(d_v + [d_v[0]], d_s + [d_s[0]], d_num, d_den, n)
    with pytest.raises(RuntimeError, match=r"rc=-3.*2\^28"):
        terms(d_v[:2], d_s[:2], d_num, d_den, too_many)
    with pytest.raises(RuntimeError, match=r"rc=-3.*null.*d_num"):
        terms(d_v[:2], d_s[:2], 0, d_den, n)
    with pytest.raises(RuntimeError, match=r"rc=-3.*null.*d_den"):
        terms(d_v[:2], d_s[:2], d_num, 0, n)
    with pytest.raises(RuntimeError, match=r"rc=-3.*d_num and d_den overlap"):
        terms(d_v[:2], d_s[:2], d_num, d_num, n)
    with pytest.raises(RuntimeError, match=r"rc=-3.*d_den overlaps d_sigmas\[1\]"):
        terms(d_v[:2], d_s[:2], d_num, d_s[1], n)
    with pytest.raises(RuntimeError, match=r"rc=-3.*2\^28"):
        gpu.fr_powers(None, w, d_num, too_many)
    with pytest.raises(RuntimeError, match=r"rc=-3.*null"):
        gpu.fr_powers(None, w, 0, n)
    # n = 0 is a success that touches nothing, and nothing above launched
    terms(d_v[:2], d_s[:2], d_num, d_den, 0)
    gpu.fr_powers(None, w, d_num, 0)
    assert dev.get(d_num, n + 1) == POISON * (n + 1)
    assert dev.get(d_den, n + 1) == POISON * (n + 1)
    for p, b in zip(d_in, in_b):
        assert dev.get(p, n) == b
    # and a valid call still works
    terms(d_v, d_s, d_num, d_den, n)
    want_num, want_den = pr.terms(
        [c[:n] for c in columns["values"]], [c[:n] for c in columns["sigmas"]],
        columns["beta"], columns["gamma"], root(9), 1, DELTA, n)
    assert dev.get_guarded(d_num, n, "d_num") == pr.mont(want_num)
    assert dev.get_guarded(d_den, n, "d_den") == pr.mont(want_den)
