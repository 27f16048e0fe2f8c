"""Reference for spectre_gpu_fr_gate_eval on plain Python integers.

TEST INFRASTRUCTURE, shared by test_gate_ref.py, test_quotient_gpu.py,
test_gpu_parity.py and tools/stress_parity.py. Two independent evaluators of
one gate expression, and the header's rules for what a call is refused:

  eval_program()   the stack machine of include/spectre_gpu.h, row by row:
                   COL pushes cols[a][(row + b*rot_scale) mod n], CONST pushes
                   consts[a], ADD/SUB/MUL pop two (second-from-top OP top), NEG
                   negates the top; out = prev*y + v when y is given
  eval_tree()      the same expression as a tree, by recursion: no stack
  compile_tree()   tree -> (postfix program, its maximum stack depth); a
                   binary node needs max(d(L), 1 + d(R)) slots, as L's value
                   waits on the stack while R is computed
  right_comb()     l0 op (l1 op (... op l_{k-1})): depth k, every slot live
  random_tree()    a tree of exactly the asked depth
  check_program()  why the header refuses a call, or None

A tree is a tuple: ("col", c, rot), ("const", k), ("neg", T), or
("add" | "sub" | "mul", L, R). Values are canonical integers mod R; mont() /
ints() encode and decode the 32-byte Montgomery images the library moves,
x * 2^256 mod R little-endian, as tests/edge_operands.py has them."""
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "bn254_ref", os.path.join(HERE, "golden", "bn254_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
R, MONT = ref.R, ref.MONT
MONT_INV = pow(MONT, -1, R)

# opcodes and limits of include/spectre_gpu.h
COL, CONST, ADD, SUB, MUL, NEG = range(6)
MAX_DEPTH = 8
BINARY = {"add": ADD, "sub": SUB, "mul": MUL}


def enc(v: int) -> bytes:
    return (v % R * MONT % R).to_bytes(32, "little")


def mont(vals) -> bytes:
    return b"".join(enc(v) for v in vals)


def ints(data: bytes) -> list[int]:
    return [int.from_bytes(data[i:i + 32], "little") * MONT_INV % R
            for i in range(0, len(data), 32)]


# ------------------------------------------------------------- stack machine
def eval_program(cols, consts, program, n, rot_scale, y=None, prev=None):
    """The evaluator's semantics restated: one stack per row, rotations
    (row + rot*rot_scale) mod n, out = prev*y + v when y is given."""
    out = []
    for row in range(n):
        st = []
        for op, a, b in program:
            if op == COL:
                st.append(cols[a][(row + b * rot_scale) % n])
            elif op == CONST:
                st.append(consts[a])
            elif op == NEG:
                st[-1] = (-st[-1]) % R
            else:
                rhs = st.pop()
                lhs = st.pop()
                st.append((lhs + rhs) % R if op == ADD else
                          (lhs - rhs) % R if op == SUB else
                          lhs * rhs % R)
        v = st[0]
        if y is not None:
            v = (prev[row] * y + v) % R
        out.append(v)
    return out


def observed_depth(program) -> int:
    """The deepest stack a well-formed program reaches while it runs."""
    depth = deepest = 0
    for op, _, _ in program:
        if op in (COL, CONST):
            depth += 1
        elif op != NEG:
            depth -= 1
        deepest = max(deepest, depth)
    return deepest


# --------------------------------------------------------------------- trees
def eval_tree(tree, row, cols, consts, n, rot_scale):
    kind = tree[0]
    if kind == "col":
        return cols[tree[1]][(row + tree[2] * rot_scale) % n]
    if kind == "const":
        return consts[tree[1]]
    if kind == "neg":
        return (-eval_tree(tree[1], row, cols, consts, n, rot_scale)) % R
    lhs = eval_tree(tree[1], row, cols, consts, n, rot_scale)
    rhs = eval_tree(tree[2], row, cols, consts, n, rot_scale)
    if kind == "add":
        return (lhs + rhs) % R
    if kind == "sub":
        return (lhs - rhs) % R
    assert kind == "mul", kind
    return lhs * rhs % R


def compile_tree(tree):
    """(postfix program, maximum stack depth)."""
    kind = tree[0]
    if kind == "col":
        return [(COL, tree[1], tree[2])], 1
    if kind == "const":
        return [(CONST, tree[1], 0)], 1
    if kind == "neg":
        prog, d = compile_tree(tree[1])
        return prog + [(NEG, 0, 0)], d
    lp, ld = compile_tree(tree[1])
    rp, rd = compile_tree(tree[2])
    return lp + rp + [(BINARY[kind], 0, 0)], max(ld, 1 + rd)


def right_comb(leaves, op):
    """l0 op (l1 op (... op l_{k-1})); op is one name or one per joint."""
    ops = [op] * (len(leaves) - 1) if isinstance(op, str) else list(op)
    assert len(ops) == len(leaves) - 1
    tree = leaves[-1]
    for leaf, o in zip(reversed(leaves[:-1]), reversed(ops)):
        tree = (o, leaf, tree)
    return tree


def _random_leaf(rng, ncols, nconst, rots):
    if ncols and (not nconst or rng.random() < 0.7):
        return ("col", rng.randrange(ncols), rng.choice(rots))
    return ("const", rng.randrange(nconst))


def _random_subtree(rng, ncols, nconst, rots, max_depth, fuel):
    """A tree of compiled depth <= max_depth with at most `fuel` joints."""
    if max_depth >= 2 and fuel > 0 and rng.random() < 0.6:
        lf = rng.randrange(fuel)
        tree = (rng.choice(("add", "sub", "mul")),
                _random_subtree(rng, ncols, nconst, rots, max_depth, lf),
                _random_subtree(rng, ncols, nconst, rots, max_depth - 1,
                                fuel - 1 - lf))
    else:
        tree = _random_leaf(rng, ncols, nconst, rots)
    return ("neg", tree) if rng.random() < 0.15 else tree


def random_tree(rng, ncols, nconst, rots, depth):
    """A random tree whose compiled depth is exactly `depth`: a right comb of
    `depth` elements, element i a random subtree of depth <= depth - i. The
    comb's depth is max_i(i + d(element i)), which the last element, a leaf at
    position depth - 1, brings to `depth` and no element exceeds."""
    assert depth >= 1 and (ncols or nconst)
    elems = [_random_subtree(rng, ncols, nconst, rots, depth - i, 3)
             for i in range(depth)]
    tree = right_comb(elems, [rng.choice(("add", "sub", "mul"))
                              for _ in range(depth - 1)])
    if rng.random() < 0.3:
        tree = ("neg", tree)
    assert compile_tree(tree)[1] == depth
    return tree


# ---------------------------------------------------------- the header's rules
def check_program(program, ncols, nconst, n, rot_scale):
    """The reason include/spectre_gpu.h refuses gate_eval with this program
    and shape, or None. Rotations are taken in unbounded integers."""
    if len(program) == 0:
        return "zero ops"
    if n <= 0 or n & (n - 1):
        return "n is not a nonzero power of two"
    depth = 0
    for pc, (op, a, b) in enumerate(program):
        if op == COL:
            if a >= ncols:
                return f"column index {a} >= {ncols} at op {pc}"
            if abs(b * rot_scale) >= n:
                return f"rotation {b} * {rot_scale} out of range at op {pc}"
            depth += 1
        elif op == CONST:
            if a >= nconst:
                return f"constant index {a} >= {nconst} at op {pc}"
            depth += 1
        elif op == NEG:
            if depth < 1:
                return f"stack underflow at op {pc}"
        elif op in (ADD, SUB, MUL):
            if depth < 2:
                return f"stack underflow at op {pc}"
            depth -= 1
        else:
            return f"bad opcode {op} at op {pc}"
        if depth > MAX_DEPTH:
            return f"depth {depth} above {MAX_DEPTH} at op {pc}"
    if depth != 1:
        return f"leftover stack of {depth}"
    return None
