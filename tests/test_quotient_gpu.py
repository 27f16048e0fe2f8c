"""GPU checks of the quotient phase, spectre_gpu_fr_gate_eval and
spectre_gpu_fr_vec_op, at the edges of their contract in include/spectre_gpu.h.

The reference is tests/gate_ref.py (plain Python integers, loaded by path);
every comparison is byte-exact on Montgomery images. Every output buffer is
poisoned with 0xa5 and one element longer than the call writes, and that
element must come back untouched; every input buffer is downloaded after the
call and compared with what was uploaded. The columns live on the device for
the whole module (4096 rows; a call over n rows sees the first n) and nothing
may change them. A refused call is one that the library's host code stops
before it launches anything: the program is first put to
gate_ref.check_program, so that no call reaches a kernel with an index or a
rotation the header rules out."""
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


gr = _load("gate_ref")
edge = _load("edge_operands")
R = gr.R
COL, CONST, ADD, SUB, MUL, NEG = gr.COL, gr.CONST, gr.ADD, gr.SUB, gr.MUL, gr.NEG
POISON = b"\xa5" * 32

N_MAX = 4096
NCOLS = 40
NCONST = 64
# canonical values of the special images (0, 1, r - 1, 2^253, all-ones-low...)
SPECIALS = tuple(x * gr.MONT_INV % R for x in edge.specials(R))
assert {0, 1, R - 1} <= set(SPECIALS)


def first_diff(got: bytes, exp: bytes):
    """None when equal, else (element index, got, expected) of the first
    element that differs: a failure prints 64 bytes, not the vectors."""
    if got == exp:
        return None
    if len(got) != len(exp):
        return ("length", len(got), len(exp))
    for i in range(0, len(exp), 32):
        if got[i:i + 32] != exp[i:i + 32]:
            return (i // 32, got[i:i + 32].hex(), exp[i:i + 32].hex())


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


class Columns:
    """NCOLS device columns of N_MAX rows and a poisoned guard row: random
    values with the special images in the first rows, every image against
    every column by a per-column rotation. Also NCONST constants."""

    def __init__(self, g):
        rng = random.Random(0x90071e)
        self.g, self.dev = g, Dev(g)
        self.ints, self.bytes, self.ptr = [], [], []
        for k in range(NCOLS):
            col = [rng.randrange(R) for _ in range(N_MAX)]
            for t in range(len(SPECIALS)):
                col[t] = SPECIALS[(t + 5 * k) % len(SPECIALS)]
            self.ints.append(col)
            self.bytes.append(gr.mont(col) + POISON)
            self.ptr.append(self.dev.put(self.bytes[-1]))
        self.consts = [0, 1, R - 1] + [rng.randrange(R)
                                       for _ in range(NCONST - 3)]

    def check_unchanged(self, ids, what):
        for j in ids:
            got = self.g.download(self.ptr[j], 32 * (N_MAX + 1))
            assert first_diff(got, self.bytes[j]) is None, \
                f"{what}: column {j} was written"


@pytest.fixture(scope="module")
def cols(gpu):
    c = Columns(gpu)
    yield c
    c.dev.free()


def run_gate(cols, ids, consts, program, n, rot_scale, what, y=None,
             prev=None):
    """One accepted gate_eval over columns `ids`, compared with the
    reference; returns the expected values. With y, d_out starts as prev."""
    assert gr.check_program(program, len(ids), len(consts), n,
                            rot_scale) is None, what
    assert (y is None) == (prev is None)
    want = gr.eval_program([cols.ints[j] for j in ids], consts, program, n,
                           rot_scale, y, prev)
    d = Dev(cols.g)
    try:
        d_out = d.out(n) if prev is None else d.put(gr.mont(prev) + POISON)
        cols.g.gate_eval([cols.ptr[j] for j in ids], gr.mont(consts), program,
                         n, rot_scale=rot_scale,
                         y=None if y is None else gr.enc(y), d_out=d_out)
        got = d.get_guarded(d_out, n, what)
    finally:
        d.free()
    assert first_diff(got, gr.mont(want)) is None, what
    cols.check_unchanged(ids, what)
    return want


def flex_tree(n, rot_scale):
    """q * (a + b*c - d) at rotations {0, 1, -1, 2} where n allows them."""
    def rot(r):
        return r if abs(r * rot_scale) < n else 0
    return ("mul", ("col", 0, 0),
            ("sub", ("add", ("col", 1, rot(0)),
                     ("mul", ("col", 1, rot(1)), ("col", 2, rot(-1)))),
             ("col", 3, rot(2))))


# ------------------------------------------------------------- a. depth 1..8
@pytest.mark.parametrize("depth", range(1, gr.MAX_DEPTH + 1))
def test_gate_depth(cols, depth):
    """Every stack depth the header accepts, the deepest one included (seven
    LDS slots, 56 KiB of dynamic LDS). A right comb of SUBs over pairwise
    distinct (column, rotation) leaves keeps every slot live at once, and
    SUB makes the order of the slots matter."""
    ids = list(range(8))
    leaves = [("col", (3 * i) % 8, i - 3) for i in range(depth)]
    assert len(set(leaves)) == depth
    mixed = list(leaves)
    mixed[depth // 2] = ("neg", mixed[depth // 2])
    if depth >= 2:
        mixed[(depth // 2 + 1) % depth] = ("const", 2)
    else:
        mixed[0] = ("neg", ("const", 2))
    rng = random.Random(0xdee9 + depth)
    trees = [("comb", gr.right_comb(leaves, "sub"), 1),
             ("comb with NEG and CONST", gr.right_comb(mixed, "sub"), 1)]
    for k, rs in enumerate((1, 4, 16, 21)):
        trees.append((f"random tree {k}",
                      gr.random_tree(rng, 8, 3, (-3, -2, -1, 0, 1, 2, 3),
                                     depth), rs))
    for n in (512, 64) if depth == gr.MAX_DEPTH else (512,):
        for name, tree, rs in trees:
            prog, d = gr.compile_tree(tree)
            assert d == depth == gr.observed_depth(prog), name
            run_gate(cols, ids, cols.consts[:3], prog, n, rs,
                     f"depth {depth}, n {n}, {name}")


# --------------------------------------------------------- b. launch shapes
@pytest.mark.parametrize("n", [1, 2, 32, 64, 128, 256, 512, 4096])
def test_gate_launch_shapes(cols, n):
    """Below, at and above the 256-thread block: a partial block leaves at
    row >= n with the LDS stride still 256, and n = 1 has a mask of 0."""
    for rs in sorted({1, max(1, n // 4)}):
        prog, d = gr.compile_tree(flex_tree(n, rs))
        assert d == 4
        rots = {b for op, _, b in prog if op == COL}
        assert rots == ({0, 1, -1, 2} if 2 * rs < n else
                        {0, 1, -1} if rs < n else {0}), (n, rs)
        # columns whose row 0 holds no 0 or 1, so that n = 1 still tells a
        # wrong operator or operand order from a right one
        want = run_gate(cols, [5, 6, 7, 8], [], prog, n, rs,
                        f"flex gate, n {n}, rot_scale {rs}")
        q, a, b, c = (cols.ints[j][0] for j in (5, 6, 7, 8))
        assert len({0, 1, q, a, b, c}) == 6
        if n == 1:
            assert want == [q * (a + a * b - c) % R]
            assert want[0] not in (0, q * (c - a - a * b) % R)


# ------------------------------------------------------ c. rotation bounds
def rot_program(b):
    return gr.compile_tree(("mul", ("col", 0, 0), ("col", 1, b)))[0]


@pytest.mark.parametrize("b,rot_scale", [(255, 1), (-255, 1), (3, 85),
                                         (-3, 85), (7, 0)])
def test_gate_rotation_extremes_accepted(cols, b, rot_scale):
    """|b * rot_scale| = n - 1 on both sides, and rot_scale 0."""
    n = 256
    want = run_gate(cols, [0, 1], [], rot_program(b), n, rot_scale,
                    f"rotation {b} * {rot_scale}")
    shift = b * rot_scale
    assert abs(shift) in (0, n - 1)
    assert want == [cols.ints[0][i] * cols.ints[1][(i + shift) % n] % R
                    for i in range(n)]


def refused_gate(cols, d_cols, consts, program, n, rot_scale, match, what,
                 expect_reason=True):
    """The call raises, the poisoned d_out (256 elements and the guard) is
    untouched, and so are the columns."""
    if expect_reason:
        assert gr.check_program(program, len(d_cols), len(consts), n,
                                rot_scale) is not None, what
    d = Dev(cols.g)
    try:
        d_out = d.out(256)
        with pytest.raises(RuntimeError, match=match):
            cols.g.gate_eval(d_cols, gr.mont(consts), program, n,
                             rot_scale=rot_scale, d_out=d_out)
        assert d.get(d_out, 257) == POISON * 257, f"{what}: d_out written"
    finally:
        d.free()
    cols.check_unchanged(range(4), what)


def valid_call_after(cols, what):
    """The context still computes after a refusal."""
    prog, _ = gr.compile_tree(flex_tree(256, 1))
    run_gate(cols, [0, 1, 2, 3], [], prog, 256, 1,
             f"valid call after: {what}")


@pytest.mark.parametrize("b,rot_scale", [
    (256, 1), (-256, 1), (2, 128), (-2, 128), (-2 ** 31, 1),
    (-3, 2 ** 31), (3, 2 ** 31)])
def test_gate_rotation_past_the_bound_refused(cols, b, rot_scale):
    """One past the extreme, the most negative int32, and products that need
    64 bits: all stopped by the host's rotation check."""
    what = f"rotation {b} * {rot_scale}"
    refused_gate(cols, cols.ptr[:2], [], rot_program(b), 256, rot_scale,
                 "rc=-3: .*rotation", what)
    valid_call_after(cols, what)


# --------------------------------------------------------- d. wide and long
def test_gate_wide_and_long(cols):
    """40 columns, 64 constants, 500 terms col * const summed: about 2000
    ops at depth 3, rotations out to |3 * 85| = n - 1."""
    n, rs = 256, 85
    prog = []
    for i in range(500):
        prog += [(COL, i % NCOLS, i % 7 - 3), (CONST, i % NCONST, 0),
                 (MUL, 0, 0)]
        if i:
            prog.append((ADD, 0, 0))
    assert len(prog) == 1999 and gr.observed_depth(prog) == 3
    want = run_gate(cols, list(range(NCOLS)), cols.consts, prog, n, rs,
                    "500-term sum")
    row = 17
    assert want[row] == sum(
        cols.ints[i % NCOLS][(row + (i % 7 - 3) * rs) % n]
        * cols.consts[i % NCONST] for i in range(500)) % R


def test_gate_constant_only_without_columns(cols):
    """ncols = 0: one CONST fills every row."""
    for n in (1, 256):
        want = run_gate(cols, [], cols.consts[:5], [(CONST, 4, 0)], n, 1,
                        f"constant only, n {n}")
        assert want == [cols.consts[4]] * n


# -------------------------------------------------------- e. accumulate form
@pytest.fixture(scope="module")
def three_gates():
    rng = random.Random(0xacc)
    rots = (-2, -1, 0, 1, 2)
    return [gr.compile_tree(gr.random_tree(rng, 4, 3, rots, depth))[0]
            for depth in (3, 5, 2)]


@pytest.mark.parametrize("y", [0, 1, R - 1,
                               random.Random(0x4a11).randrange(2, R - 1)],
                         ids=["0", "1", "r-1", "random"])
def test_gate_accumulate_chain(cols, three_gates, y):
    """h = (g0*y + g1)*y + g2 as three calls on one running buffer."""
    n, rs, ids, consts = 512, 2, [0, 1, 2, 3], cols.consts[:3]
    h = run_gate(cols, ids, consts, three_gates[0], n, rs, f"g0, y {y}")
    g = [gr.eval_program([cols.ints[j] for j in ids], consts, p, n, rs)
         for p in three_gates]
    assert h == g[0]
    for k in (1, 2):
        h = run_gate(cols, ids, consts, three_gates[k], n, rs,
                     f"g{k}, y {y}", y=y, prev=h)
    assert h == [((a * y + b) * y + c) % R for a, b, c in zip(*g)]


# ------------------------------------------------------------------ f. vec_op
VEC_N = [0, 1, 63, 64, 255, 256, 257, 4097]
ARRANGEMENTS = ["distinct", "out == a", "out == b", "a == b",
                "out == a == b"]


@pytest.fixture(scope="module")
def operands():
    """Two vectors of 4097 canonical values, the special images in their
    first rows (b's rotated, so that the pairs differ), and the scalars."""
    rng = random.Random(0x7ec0)
    nmax = max(VEC_N)
    a = [rng.randrange(R) for _ in range(nmax)]
    b = [rng.randrange(R) for _ in range(nmax)]
    k = len(SPECIALS)
    a[:k] = SPECIALS
    b[:k] = SPECIALS[7:] + SPECIALS[:7]
    return {"a": a, "b": b, "a_bytes": gr.mont(a), "b_bytes": gr.mont(b),
            "c": [rng.randrange(R), 0, 1, R - 1]}


def vec_expect(op, a, b, c):
    if op == 0:
        return [(x + y) % R for x, y in zip(a, b)]
    if op == 1:
        return [(x - y) % R for x, y in zip(a, b)]
    if op == 2:
        return [x * y % R for x, y in zip(a, b)]
    if op == 3:
        return [x * c % R for x in a]
    assert op == 4
    return [(x + c * y) % R for x, y in zip(a, b)]


def run_vec_op(g, operands, op, arrangement, c, n):
    what = f"op {op}, {arrangement}, n {n}, c {c}"
    a_bytes = operands["a_bytes"][:32 * n] + POISON
    b_bytes = operands["b_bytes"][:32 * n] + POISON
    a, b = operands["a"][:n], operands["b"][:n]
    d = Dev(g)
    try:
        pa = d.put(a_bytes)
        pb = pa if "a == b" in arrangement else d.put(b_bytes)
        if "a == b" in arrangement:
            b, b_bytes = a, a_bytes
        po = (pa if "out == a" in arrangement else
              pb if arrangement == "out == b" else d.out(n))
        g.fr_vec_op(op, pa, pb, gr.enc(c) if op >= 3 else None, po, n)
        got = d.get_guarded(po, n, what)
        assert first_diff(got, gr.mont(vec_expect(op, a, b, c))) is None, what
        if pa != po:
            assert d.get(pa, n + 1) == a_bytes, f"{what}: a was written"
        if pb != po:
            assert d.get(pb, n + 1) == b_bytes, f"{what}: b was written"
    finally:
        d.free()


@pytest.mark.parametrize("n", VEC_N)
def test_vec_op(gpu, operands, n):
    """All five ops under every pointer arrangement the header allows. With
    a == b SUB gives zero and MUL squares. n = 0 succeeds and writes nothing
    (the guard is then element 0)."""
    assert gpu.VEC_ADD_SCALED == 4
    for op in range(5):
        for arrangement in ARRANGEMENTS:
            cs = operands["c"] if arrangement == "distinct" and op >= 3 \
                else operands["c"][:1]
            for c in cs:
                run_vec_op(gpu, operands, op, arrangement, c, n)
    if n:
        a = operands["a"][:n]
        assert vec_expect(1, a, a, 0) == [0] * n


# --------------------------------------------------------------- g. refusals
FLEX = gr.compile_tree(flex_tree(256, 1))[0]
NINE_DEEP = gr.compile_tree(gr.right_comb([("col", 0, 0)] * 9, "add"))[0]
# (what, program, ncols, nconst, n, the library's words)
MALFORMED = [
    ("zero ops", [], 4, 0, 256, "rc=-1: .*bad arguments"),
    ("binary op on an empty stack", [(ADD, 0, 0)], 4, 0, 256,
     "rc=-3: .*underflow"),
    ("binary op on one value", [(COL, 0, 0), (MUL, 0, 0)], 4, 0, 256,
     "rc=-3: .*underflow"),
    ("NEG on an empty stack", [(NEG, 0, 0)], 4, 0, 256,
     "rc=-3: .*empty stack"),
    ("opcode 6", [(COL, 0, 0), (6, 0, 0)], 4, 0, 256, "rc=-3: .*bad opcode"),
    ("opcode 2^32 - 1", [(0xffffffff, 0, 0)], 4, 0, 256,
     "rc=-3: .*bad opcode"),
    ("column index = ncols", [(COL, 4, 0)], 4, 0, 256, "rc=-3: .*col 4 >= 4"),
    ("column index with ncols 0", [(COL, 0, 0)], 0, 1, 256,
     "rc=-3: .*col 0 >= 0"),
    ("constant index = nconst", [(CONST, 3, 0)], 4, 3, 256,
     "rc=-3: .*const 3 >= 3"),
    ("constant index with nconst 0", [(CONST, 0, 0)], 4, 0, 256,
     "rc=-3: .*const 0 >= 0"),
    ("two values left", [(COL, 0, 0), (COL, 1, 0)], 4, 0, 256,
     "rc=-3: .*leaves 2 values"),
    ("depth 9", NINE_DEEP, 4, 0, 256, "rc=-3: .*stack depth 9 > 8"),
    ("n = 0", FLEX, 4, 0, 0, "rc=-3: .*power of two"),
    ("n = 255", FLEX, 4, 0, 255, "rc=-3: .*power of two"),
    ("n = 192", FLEX, 4, 0, 192, "rc=-3: .*power of two"),
    ("rotation 1 at n = 1", [(COL, 0, 1)], 4, 0, 1, "rc=-3: .*rotation"),
]


@pytest.mark.parametrize("case", range(len(MALFORMED)),
                         ids=[m[0] for m in MALFORMED])
def test_gate_malformed_call_refused(cols, case):
    what, program, ncols, nconst, n, match = MALFORMED[case]
    refused_gate(cols, cols.ptr[:ncols], cols.consts[:nconst], program, n, 1,
                 match, what)
    valid_call_after(cols, what)


@pytest.mark.parametrize("d_cols_of,what", [
    (lambda p: [p[0], 0, p[2], p[3]], "NULL column that the program reads"),
    (lambda p: p[:4] + [0], "NULL column that the program does not read"),
    (lambda p: [0] + p[:4], "NULL first column, program reads columns 0..3"),
], ids=["read", "unread", "first"])
def test_gate_null_column_refused(cols, d_cols_of, what):
    refused_gate(cols, d_cols_of(cols.ptr), [], FLEX, 256, 1,
                 "rc=-1: .*null device pointer in d_cols", what,
                 expect_reason=False)
    valid_call_after(cols, what)


@pytest.mark.parametrize("kind", ["d_out is a column",
                                  "d_out 32 bytes into a column",
                                  "a column starts inside d_out",
                                  "d_out is a column the program skips"])
def test_gate_output_overlapping_a_column_refused(cols, kind):
    """Any byte shared between d_out[0..n) and a column's n rows, equality
    included: with a rotation a lane would read rows that others write."""
    n = 256
    rng = random.Random(0x0e71a9)
    data = gr.mont([rng.randrange(R) for _ in range(2 * n)]) + POISON
    prog = gr.compile_tree(("mul", ("col", 0, 0), ("col", 1, 1)))[0]
    d = Dev(cols.g)
    try:
        buf = d.put(data)
        d_cols, d_out = {
            "d_out is a column": ([cols.ptr[0], buf], buf),
            "d_out 32 bytes into a column": ([cols.ptr[0], buf], buf + 32),
            "a column starts inside d_out":
                ([cols.ptr[0], buf + 32 * (n - 1)], buf),
            "d_out is a column the program skips":
                ([cols.ptr[0], cols.ptr[1], buf], buf),
        }[kind]
        with pytest.raises(RuntimeError, match="rc=-1: .*d_out overlaps"):
            cols.g.gate_eval(d_cols, b"", prog, n, rot_scale=1, d_out=d_out)
        assert d.get(buf, 2 * n + 1) == data, f"{kind}: buffer written"
        # the nearest arrangement that shares no byte is accepted
        d_far = buf + 32 * n
        cols.g.gate_eval([cols.ptr[0], buf], b"", prog, n, rot_scale=1,
                         d_out=d_far)
        got = d.get(buf, 2 * n + 1)
        col = gr.ints(data[:32 * n])
        want = [cols.ints[0][i] * col[(i + 1) % n] % R for i in range(n)]
        assert got[:32 * n] == data[:32 * n], f"{kind}: column written"
        assert got[64 * n:] == POISON, f"{kind}: wrote past element {n}"
        assert first_diff(got[32 * n:64 * n], gr.mont(want)) is None, kind
    finally:
        d.free()
    cols.check_unchanged(range(2), kind)


VEC_REFUSED = [
    ("op -1", -1, "a", "b", True),
    ("op 5", 5, "a", "b", True),
    ("NULL d_a", 0, None, "b", False),
    ("NULL d_a, SCALE", 3, None, None, True),
    ("NULL d_b, ADD", 0, "a", None, False),
    ("NULL d_b, SUB", 1, "a", None, False),
    ("NULL d_b, MUL", 2, "a", None, False),
    ("NULL d_b, ADD_SCALED", 4, "a", None, True),
    ("NULL c, SCALE", 3, "a", None, False),
    ("NULL c, ADD_SCALED", 4, "a", "b", False),
]


@pytest.mark.parametrize("case", range(len(VEC_REFUSED)),
                         ids=[v[0] for v in VEC_REFUSED])
def test_vec_op_bad_arguments_refused(gpu, operands, case):
    what, op, use_a, use_b, with_c = VEC_REFUSED[case]
    n = 257
    a_bytes = operands["a_bytes"][:32 * n] + POISON
    b_bytes = operands["b_bytes"][:32 * n] + POISON
    d = Dev(gpu)
    try:
        pa, pb, po = d.put(a_bytes), d.put(b_bytes), d.out(n)
        with pytest.raises(RuntimeError, match="rc=-1: .*bad op/arguments"):
            gpu.fr_vec_op(op, pa if use_a else 0, pb if use_b else None,
                          gr.enc(operands["c"][0]) if with_c else None, po, n)
        assert d.get(po, n + 1) == POISON * (n + 1), f"{what}: d_out written"
        assert d.get(pa, n + 1) == a_bytes and d.get(pb, n + 1) == b_bytes
    finally:
        d.free()
    run_vec_op(gpu, operands, 4, "distinct", operands["c"][0], n)


def test_vec_op_null_output_refused(gpu, operands):
    n = 64
    d = Dev(gpu)
    try:
        pa = d.put(operands["a_bytes"][:32 * n] + POISON)
        with pytest.raises(RuntimeError, match="rc=-1: .*bad op/arguments"):
            gpu.fr_vec_op(0, pa, pa, None, 0, n)
        assert d.get(pa, n + 1) == operands["a_bytes"][:32 * n] + POISON
    finally:
        d.free()
    run_vec_op(gpu, operands, 0, "distinct", 0, n)
