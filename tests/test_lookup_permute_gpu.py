"""GPU checks of spectre_gpu_fr_lookup_permute, byte-exact against the serial
halo2 form in tests/lookup_permute_ref.py (plain Python integers).

Field elements come from one oracle.gen_fr_vector pool, generated and decoded
once; tables and inputs are index choices into it, so a case costs a sort on
the host and one call on the device. Output buffers carry one element more
than u, pre-filled with a pattern that has to survive, and the inputs are read
back after every call."""
import random

import pytest

import lookup_permute_ref as lp

pytestmark = pytest.mark.gpu

R = lp.R
FILL = b"\xa5" * 32
N_POOL = 65537 + 300
SIZES = [0, 1, 2, 255, 256, 257, 4097, 65537 + 300]


@pytest.fixture(scope="module")
def pool(oracle):
    """(bytes, ints) of N_POOL random field elements."""
    raw = oracle.gen_fr_vector(N_POOL, seed=6301)
    return raw, lp.ints(raw)


@pytest.fixture(scope="module")
def g():
    from spectre_amd import SpectreGpu
    ctx = SpectreGpu([0])
    yield ctx
    ctx.close()


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


def permute(g, a_b: bytes, s_b: bytes):
    """One call on fresh buffers -> (A' bytes, S' bytes). Checks that element
    u of both outputs keeps the pattern and that the inputs are unchanged,
    whether the call succeeds or raises."""
    u = len(a_b) // 32
    assert len(s_b) == 32 * u
    d = Dev(g)
    try:
        d_a, d_s = d.put(a_b), d.put(s_b)
        d_ap, d_sp = d.put(FILL * (u + 1)), d.put(FILL * (u + 1))
        try:
            g.fr_lookup_permute(d_a, d_s, d_ap, d_sp, u)
        finally:
            assert d.get(d_a, u) == a_b, "the input column was written"
            assert d.get(d_s, u) == s_b, "the table column was written"
            ap, sp = d.get(d_ap, u + 1), d.get(d_sp, u + 1)
            assert ap[32 * u:] == FILL, "A' written past u"
            assert sp[32 * u:] == FILL, "S' written past u"
    finally:
        d.free()
    return ap[:32 * u], sp[:32 * u]


def check(g, a, s, what=""):
    """Device result == the serial reference, for integer columns a, s."""
    want_a, want_s = lp.serial(a, s)
    got_a, got_s = permute(g, lp.mont(a), lp.mont(s))
    assert got_a == lp.mont(want_a), f"A' differs {what}"
    assert got_s == lp.mont(want_s), f"S' differs {what}"
    return want_a, want_s


def drawn(rng, values, u):
    """A table of u entries over `values`, every value present when u allows
    it, and u inputs drawn from that table with repeats."""
    table = [values[i % len(values)] for i in range(u)]
    rng.shuffle(table)
    return [rng.choice(table) for _ in range(u)], table


def test_reference_matches_library_encoding(oracle, pool):
    raw, vals = pool
    assert lp.mont(vals[:8]) == raw[:256]
    assert oracle.fr_mul(raw[:32], raw[32:64]) == lp.enc(vals[0] * vals[1])


@pytest.mark.parametrize("u", SIZES)
def test_sizes(g, pool, u):
    """Random full-range keys; about u/3 distinct table values, so the table
    has duplicates, the inputs repeat and some table values stay unused.
    From u = 255 on the case is also shown to tell the canonical order from
    the order of the stored (Montgomery) bytes."""
    raw, vals = pool
    rng = random.Random(6400 + u)
    k = max(1, u // 3)
    t_idx = [rng.randrange(k) for _ in range(u)]
    a_idx = [rng.choice(t_idx) for _ in range(u)]
    a_b = b"".join(raw[32 * i:32 * i + 32] for i in a_idx)
    s_b = b"".join(raw[32 * i:32 * i + 32] for i in t_idx)
    want_a, want_s = lp.serial([vals[i] for i in a_idx],
                               [vals[i] for i in t_idx])
    got_a, got_s = permute(g, a_b, s_b)
    assert got_a == lp.mont(want_a), f"A' differs at u={u}"
    assert got_s == lp.mont(want_s), f"S' differs at u={u}"
    if u >= 255:
        by_bytes = sorted(a_b[i:i + 32][::-1] for i in range(0, len(a_b), 32))
        assert got_a != b"".join(x[::-1] for x in by_bytes), \
            "the case does not tell canonical from Montgomery order"


def test_order_is_canonical_not_montgomery(g):
    """1 < 4, but 4 * (2^256 mod R) wraps past R once, which leaves the
    Montgomery image of 4 below that of 1: a sort of the stored bytes swaps
    them."""
    lo, hi = 1, 4
    as_stored = [int.from_bytes(lp.enc(v), "little") for v in (lo, hi)]
    assert as_stored[0] > as_stored[1], "pick another pair"
    got_a, got_s = permute(g, lp.mont([hi, lo]), lp.mont([lo, hi]))
    assert got_a == lp.mont([lo, hi])
    assert got_s == lp.mont([lo, hi])
    check(g, [hi, lo, hi, hi, lo], [hi, lo, lo, hi, hi], "(1, 4)")


def key_sets(vals):
    low192 = vals[0] % (1 << 192)
    high = (vals[1] >> 64 << 64) % R
    assert high >> 64, "the common high part has to be nonzero"
    sets = {}
    for name, top in (("max_2^19-1", (1 << 19) - 1),
                      ("max_2^64-1", (1 << 64) - 1), ("max_2^64", 1 << 64),
                      ("max_2^128", 1 << 128), ("max_2^192", 1 << 192),
                      ("max_R-1", R - 1)):
        sets[name] = sorted({top, top - 1, top // 2, top // 3, 0, 1, 5}
                            | {v % (top + 1) for v in vals[2:22]})
    # equal low three limbs, only the top limb differs (all below R)
    sets["top_limb_only"] = [low192 + (t << 192)
                             for t in (0, 1, 2, 3, 0x1000, (R >> 192) - 1)]
    # a common nonzero high part, only limb 0 differs
    sets["limb0_only"] = [high + t for t in
                          (0, 1, 2, 1 << 31, 1 << 32, 1 << 63, (1 << 64) - 1,
                           vals[22] % (1 << 64), vals[23] % (1 << 64))]
    sets["zero_and_R-1"] = [0, R - 1, 1, R - 2, vals[24], vals[25]]
    return sets


KEY_SET_NAMES = ["max_2^19-1", "max_2^64-1", "max_2^64", "max_2^128",
                 "max_2^192", "max_R-1", "top_limb_only", "limb0_only",
                 "zero_and_R-1"]


@pytest.mark.parametrize("name", KEY_SET_NAMES)
def test_key_widths(g, pool, name):
    """The sort skips limbs and bits that are zero everywhere; every width
    has to give the bytes of the full sort. 300 rows: more than one block."""
    values = key_sets(pool[1])[name]
    assert all(0 <= v < R for v in values) and len(set(values)) == len(values)
    rng = random.Random(len(name) * 131 + len(values))
    a, s = drawn(rng, values, 300)
    check(g, a, s, name)


def test_shape_all_inputs_equal(g, pool):
    vals = pool[1]
    u = 1000
    s = [vals[i % 50] for i in range(u)]
    want_a, want_s = check(g, [vals[7]] * u, s, "all inputs equal")
    assert want_s[0] == vals[7] and len(set(want_a)) == 1


def test_shape_permutation_of_duplicate_free_table(g, pool):
    vals = pool[1]
    u = 1500
    s = vals[:u]
    assert len(set(s)) == u
    a = s[:]
    random.Random(6501).shuffle(a)
    want_a, want_s = check(g, a, s, "permutation")
    assert want_s == want_a  # no repeated rows


def test_shape_constant_table(g, pool):
    v = pool[1][9]
    check(g, [v] * 777, [v] * 777, "constant table")
    check(g, [0] * 300, [0] * 300, "all zero")


def test_shape_range_check(g):
    """The range-check lookup: table i mod 2^12, 12-bit keys, one short
    sort pass."""
    u = 3 * 4096 + 5
    rng = random.Random(6502)
    check(g, [rng.randrange(4096) for _ in range(u)],
          [i % 4096 for i in range(u)], "range check")


def miss_cases(vals):
    """(name, inputs, table, distinct missing) over a full-range table."""
    tab = sorted(set(vals[100:160]))
    assert tab[0] > 0 and tab[-1] < R - 1
    between = next(v + 1 for v in tab if v + 1 not in tab)
    assert tab[0] < between < tab[-1]
    rng = random.Random(6503)
    a0, s = drawn(rng, tab, 300)
    cases = []
    for name, bad in (("below", [tab[0] - 1]), ("above", [tab[-1] + 1]),
                      ("between", [between]),
                      ("several", [tab[0] - 1, between, between,
                                   tab[-1] + 1, 0])):
        a = a0[:]
        for k, v in enumerate(bad):
            a[17 + 40 * k] = v
        cases.append((name, a, s, len(set(bad))))
    return cases


@pytest.mark.parametrize("which", [0, 1, 2, 3],
                         ids=["below", "above", "between", "several"])
def test_miss(g, pool, which):
    from spectre_amd import SpectreGpu
    name, a, s, missing = miss_cases(pool[1])[which]
    with pytest.raises(lp.LookupMiss) as ref_err:
        lp.serial(a, s)
    assert ref_err.value.missing == missing
    assert SpectreGpu.ERR_LOOKUP_MISS == -5
    plural = "" if missing == 1 else "s"
    with pytest.raises(
            RuntimeError,
            match=rf"rc=-5: .*lookup miss: {missing} distinct input "
                  rf"value{plural} absent"):
        permute(g, lp.mont(a), lp.mont(s))  # also: inputs untouched
    # the same context still answers a valid call correctly
    in_table = set(s)
    good = [v if v in in_table else s[0] for v in a]
    check(g, good, s, f"after miss {name}")


def test_rejected_calls(g, pool):
    raw = pool[0]
    u = 64
    a_b, s_b = raw[:32 * u], raw[32 * u:64 * u]
    d = Dev(g)
    bufs = [d.put(a_b), d.put(s_b), d.put(FILL * u), d.put(FILL * u)]
    for i in range(4):
        args = bufs[:]
        args[i] = 0
        with pytest.raises(RuntimeError, match="null"):
            g.fr_lookup_permute(*args, u)
    with pytest.raises(RuntimeError, match=r"2\^28"):
        g.fr_lookup_permute(*bufs, (1 << 28) + 1)
    with pytest.raises(RuntimeError, match="invalid ctx/device"):
        g.fr_lookup_permute(*bufs, u, dev=7)
    for i in range(4):
        for j in range(i + 1, 4):
            for shift in (0, 32 * (u - 1)):  # the same range; one element
                args = bufs[:]
                args[j] = bufs[i] + shift
                with pytest.raises(RuntimeError, match="overlap"):
                    g.fr_lookup_permute(*args, u)
                args = bufs[:]
                args[i] = bufs[j] + shift
                with pytest.raises(RuntimeError, match="overlap"):
                    g.fr_lookup_permute(*args, u)
    # nothing was written by any of them
    assert d.get(bufs[0], u) == a_b and d.get(bufs[1], u) == s_b
    assert d.get(bufs[2], u) == FILL * u and d.get(bufs[3], u) == FILL * u
    d.free()


def test_adjacent_ranges_and_determinism(g, pool):
    """Four touching quarters of one allocation are no overlap; and two calls
    give identical bytes."""
    raw, vals = pool
    u = 4097
    rng = random.Random(6504)
    t_idx = [rng.randrange(900) for _ in range(u)]
    a_idx = [rng.choice(t_idx) for _ in range(u)]
    a_b = b"".join(raw[32 * i:32 * i + 32] for i in a_idx)
    s_b = b"".join(raw[32 * i:32 * i + 32] for i in t_idx)
    want_a, want_s = lp.serial([vals[i] for i in a_idx],
                               [vals[i] for i in t_idx])
    d = Dev(g)
    one = d.put(a_b + s_b + FILL * (2 * u))
    q = [one + 32 * u * k for k in range(4)]
    g.fr_lookup_permute(*q, u)
    first = d.get(one, 4 * u)
    assert first == a_b + s_b + lp.mont(want_a) + lp.mont(want_s)
    g.upload(q[2], FILL * (2 * u))
    g.fr_lookup_permute(*q, u)
    assert d.get(one, 4 * u) == first
    d.free()
    assert permute(g, a_b, s_b) == (first[64 * u:96 * u], first[96 * u:])


def test_chain_grand_product_and_commit(g, oracle, pool):
    """permute -> the lookup Z column's grand product ends at one (halo2's
    own assertion), and the commitment of the device's A' equals that of the
    host-sorted column uploaded."""
    raw, vals = pool
    u = 4096
    rng = random.Random(6505)
    t_idx = [rng.randrange(700) for _ in range(u)]
    a_idx = [rng.choice(t_idx) for _ in range(u)]
    a = [vals[i] for i in a_idx]
    s = [vals[i] for i in t_idx]
    beta, gamma = vals[-1], vals[-2]
    _, bases = oracle.gen_msm_inputs(u, seed=6506, fast=True)
    d = Dev(g)
    d_a, d_s = d.put(lp.mont(a)), d.put(lp.mont(s))
    d_ap, d_sp = d.put(FILL * u), d.put(FILL * u)
    g.fr_lookup_permute(d_a, d_s, d_ap, d_sp, u)
    ap, sp = lp.ints(d.get(d_ap, u)), lp.ints(d.get(d_sp, u))
    num = [(a[i] + beta) * (s[i] + gamma) % R for i in range(u)]
    den = [(ap[i] + beta) * (sp[i] + gamma) % R for i in range(u)]
    assert 0 not in den
    d_num, d_den, d_z = d.put(lp.mont(num)), d.put(lp.mont(den)), \
        d.put(FILL * u)
    last = g.fr_grand_product(d_num, d_den, None, d_z, u)
    assert last == lp.enc(1), "the lookup product does not close"
    d_bases = d.put(bases)
    d_sorted = d.put(lp.mont(sorted(a)))
    got = g.msm_device(d_bases, d_ap, u, canonical=False)
    want = g.msm_device(d_bases, d_sorted, u, canonical=False)
    d.free()
    assert got == want, "commitments differ"
    assert got != bytes(64)
