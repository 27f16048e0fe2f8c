"""CPU checks of tests/gate_ref.py: the stack machine against the recursive
tree evaluator, the depth rule, the exact-depth generator, and the refusal
rules of include/spectre_gpu.h at the cases test_quotient_gpu.py sends."""
import importlib.util
import os
import random

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "gate_ref", os.path.join(HERE, "gate_ref.py"))
gr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gr)
R = gr.R
COL, CONST, ADD, SUB, MUL, NEG = gr.COL, gr.CONST, gr.ADD, gr.SUB, gr.MUL, gr.NEG

N = 16
NCOLS, NCONST = 4, 3
ROTS = (-3, -2, -1, 0, 1, 2, 3)


@pytest.fixture(scope="module")
def data():
    rng = random.Random(0x6a7e)
    cols = [[rng.randrange(R) for _ in range(N)] for _ in range(NCOLS)]
    cols[0][:4] = [0, 1, R - 1, 2]
    return cols, [rng.randrange(R) for _ in range(NCONST)]


def test_header_constants_match():
    with open(os.path.join(HERE, "..", "include", "spectre_gpu.h")) as f:
        text = f.read()
    for name, val in (("OP_COL", COL), ("OP_CONST", CONST), ("OP_ADD", ADD),
                      ("OP_SUB", SUB), ("OP_MUL", MUL), ("OP_NEG", NEG),
                      ("MAX_DEPTH", gr.MAX_DEPTH)):
        assert f"#define SPECTRE_GATE_{name} {val}\n" in text, name


def test_mont_round_trip():
    xs = [0, 1, 2, R - 1, R - 2, 1 << 253, random.Random(5).randrange(R)]
    assert gr.ints(gr.mont(xs)) == xs
    assert gr.enc(1) == (gr.MONT % R).to_bytes(32, "little")
    assert gr.enc(R + 5) == gr.enc(5)


def test_hand_written_program(data):
    """q * (a + b*c - d) both ways, against the formula written out."""
    cols, consts = data
    tree = ("mul", ("col", 0, 0),
            ("sub", ("add", ("col", 1, 0),
                     ("mul", ("col", 1, 1), ("col", 2, -1))),
             ("const", 1)))
    prog, depth = gr.compile_tree(tree)
    assert depth == 4
    assert prog == [(COL, 0, 0), (COL, 1, 0), (COL, 1, 1), (COL, 2, -1),
                    (MUL, 0, 0), (ADD, 0, 0), (CONST, 1, 0), (SUB, 0, 0),
                    (MUL, 0, 0)]
    for rs in (1, 2):
        want = [cols[0][i] * (cols[1][i] + cols[1][(i + rs) % N]
                              * cols[2][(i - rs) % N] - consts[1]) % R
                for i in range(N)]
        assert gr.eval_program(cols, consts, prog, N, rs) == want
        assert [gr.eval_tree(tree, i, cols, consts, N, rs)
                for i in range(N)] == want
    y, prev = 12345, list(range(100, 100 + N))
    assert gr.eval_program(cols, consts, prog, N, 2, y, prev) == \
        [(p * y + w) % R for p, w in zip(prev, want)]


def test_sub_and_neg_order():
    cols, consts = [[7]], [3]
    assert gr.eval_program(cols, consts, [(COL, 0, 0), (CONST, 0, 0),
                                          (SUB, 0, 0)], 1, 1) == [4]
    assert gr.eval_program(cols, consts, [(CONST, 0, 0), (COL, 0, 0),
                                          (SUB, 0, 0)], 1, 1) == [R - 4]
    assert gr.eval_program(cols, consts, [(COL, 0, 0), (NEG, 0, 0)],
                           1, 1) == [R - 7]


def test_stack_machine_agrees_with_tree_evaluation(data):
    cols, consts = data
    rng = random.Random(0x7ee5)
    for seed in range(240):
        depth = 1 + seed % 8
        tree = gr.random_tree(rng, NCOLS, NCONST, ROTS, depth)
        prog, d = gr.compile_tree(tree)
        rs = rng.choice((0, 1, 2, 5))
        got = gr.eval_program(cols, consts, prog, N, rs)
        want = [gr.eval_tree(tree, i, cols, consts, N, rs) for i in range(N)]
        assert got == want, (seed, tree)
        assert gr.check_program(prog, NCOLS, NCONST, N, rs) is None


@pytest.mark.parametrize("depth", range(1, 9))
def test_random_tree_has_exactly_the_asked_depth(depth):
    """Every tree, not a sample of them: the compiled depth, the depth seen
    while running the program, and the asked depth are one number."""
    rng = random.Random(0xd0 + depth)
    for k in range(60):
        ncols, nconst = ((3, 2), (1, 0), (0, 2))[k % 3]
        tree = gr.random_tree(rng, ncols, nconst, (-1, 0, 2), depth)
        prog, d = gr.compile_tree(tree)
        assert d == depth
        assert gr.observed_depth(prog) == depth
        assert all(a < max(ncols, 1) for op, a, _ in prog if op == COL)
        assert not (ncols == 0 and any(op == COL for op, _, _ in prog))
        assert not (nconst == 0 and any(op == CONST for op, _, _ in prog))


@pytest.mark.parametrize("k", range(1, 9))
def test_right_comb_depth_and_value(k):
    leaves = [("col", 0, i) for i in range(k)]
    tree = gr.right_comb(leaves, "sub")
    prog, d = gr.compile_tree(tree)
    assert d == k == gr.observed_depth(prog)
    assert [op for op, _, _ in prog] == [COL] * k + [SUB] * (k - 1)
    col = [3 ** i for i in range(N)]
    # l0 - (l1 - (l2 - ...)) is the alternating sum
    want = [sum((-1) ** i * col[(r + i) % N] for i in range(k)) % R
            for r in range(N)]
    assert gr.eval_program([col], [], prog, N, 1) == want
    # the left comb of the same leaves needs two slots however long it is
    left = leaves[0]
    for leaf in leaves[1:]:
        left = ("sub", left, leaf)
    assert gr.compile_tree(left)[1] == min(k, 2)


def _comb(k):
    return gr.compile_tree(
        gr.right_comb([("col", 0, 0)] * k, "add"))[0]


MALFORMED = [
    ("zero ops", [], 256, 1),
    ("underflow", [(ADD, 0, 0)], 256, 1),
    ("underflow", [(COL, 0, 0), (MUL, 0, 0)], 256, 1),
    ("underflow", [(NEG, 0, 0)], 256, 1),
    ("bad opcode", [(COL, 0, 0), (6, 0, 0)], 256, 1),
    ("bad opcode", [(0xffffffff, 0, 0)], 256, 1),
    ("column index", [(COL, 2, 0)], 256, 1),
    ("constant index", [(CONST, 3, 0)], 256, 1),
    ("leftover", [(COL, 0, 0), (COL, 1, 0)], 256, 1),
    ("depth", _comb(9), 256, 1),
    ("power of two", [(COL, 0, 0)], 0, 1),
    ("power of two", [(COL, 0, 0)], 255, 1),
    ("power of two", [(COL, 0, 0)], 768, 1),
    ("rotation", [(COL, 0, 256)], 256, 1),
    ("rotation", [(COL, 0, -256)], 256, 1),
    ("rotation", [(COL, 0, 2)], 256, 128),
    ("rotation", [(COL, 0, -2)], 256, 128),
    ("rotation", [(COL, 0, -2 ** 31)], 256, 1),
    ("rotation", [(COL, 0, -3)], 256, 2 ** 31),
    ("rotation", [(COL, 0, 3)], 256, 2 ** 31),
    ("rotation", [(COL, 0, 1)], 1, 1),
]


@pytest.mark.parametrize("case", range(len(MALFORMED)))
def test_check_program_names_the_class(case):
    word, prog, n, rs = MALFORMED[case]
    reason = gr.check_program(prog, 2, 3, n, rs)
    assert reason is not None and word in reason, reason


def test_check_program_accepts_the_boundaries():
    for b, rs in ((255, 1), (-255, 1), (3, 85), (-3, 85), (7, 0),
                  (-2 ** 31, 0)):
        assert gr.check_program([(COL, 1, b)], 2, 0, 256, rs) is None, (b, rs)
    assert gr.check_program(_comb(8), 1, 0, 256, 1) is None
    assert gr.check_program([(CONST, 0, 0)], 0, 1, 256, 1) is None
    assert gr.check_program([(COL, 0, 0)], 1, 0, 1, 1) is None
    assert gr.check_program([(COL, 0, 0), (NEG, 0, 0)], 1, 0, 2, 5) is None
