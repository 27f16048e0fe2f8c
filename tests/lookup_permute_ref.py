"""Reference for spectre_gpu_fr_lookup_permute on plain Python integers.

Two forms of halo2's permute_expression_pair over u rows of a lookup's
compressed input column A and table column S:

  serial()    the published algorithm: sort A, count S in an ordered map, walk
              A' upward (a first occurrence takes its value out of the map,
              every other row joins the list of repeated rows), then hand the
              values left in the map, ascending, to the rows popped from the
              END of that list;
  parallel()  the form the device runs: lower bounds of the first rows in the
              sorted table, two compactions, one reversed scatter.

Both return (A', S') or raise LookupMiss carrying the number of distinct input
values the table does not hold. Values are canonical integers; ints() / mont()
decode and encode the 32-byte Montgomery images the library moves, with
tests/golden/bn254_ref.py loaded by path."""
import bisect
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "bn254_ref", os.path.join(HERE, "golden", "bn254_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
R = ref.R
MONT_INV = pow(ref.MONT, -1, R)


class LookupMiss(Exception):
    def __init__(self, missing: int):
        super().__init__(f"{missing} distinct input values not in the table")
        self.missing = missing


def ints(data: bytes) -> list[int]:
    return [int.from_bytes(data[i:i + 32], "little") * MONT_INV % R
            for i in range(0, len(data), 32)]


def enc(v: int) -> bytes:
    return ref.to_mont_bytes(v % R, R)


def mont(vals) -> bytes:
    return b"".join(enc(v) for v in vals)


def serial(a, s):
    """halo2's walk. The whole of A' is walked before a miss is raised, so the
    count covers every distinct missing value (halo2 itself stops at the
    first)."""
    assert len(a) == len(s)
    a_perm = sorted(a)
    counts = {}
    for v in s:
        counts[v] = counts.get(v, 0) + 1
    s_perm = [None] * len(a)
    repeated = []
    missing = 0
    for row, v in enumerate(a_perm):
        if row == 0 or v != a_perm[row - 1]:
            if counts.get(v, 0) == 0:
                missing += 1
                continue
            s_perm[row] = v
            counts[v] -= 1
        else:
            repeated.append(row)
    if missing:
        raise LookupMiss(missing)
    for v in sorted(counts):
        for _ in range(counts[v]):
            s_perm[repeated.pop()] = v
    assert not repeated
    return a_perm, s_perm


def parallel(a, s):
    """The same result from a sort, lower bounds and two compactions."""
    assert len(a) == len(s)
    u = len(a)
    a_perm = sorted(a)
    ss = sorted(s)
    first = [i == 0 or a_perm[i] != a_perm[i - 1] for i in range(u)]
    taken = [False] * u
    missing = 0
    for i in range(u):
        if not first[i]:
            continue
        p = bisect.bisect_left(ss, a_perm[i])
        if p == u or ss[p] != a_perm[i]:
            missing += 1
        else:
            assert not taken[p]
            taken[p] = True
    if missing:
        raise LookupMiss(missing)
    left = [ss[p] for p in range(u) if not taken[p]]
    rep = [i for i in range(u) if not first[i]]
    m = len(rep)
    assert len(left) == m
    s_perm = [a_perm[i] if first[i] else None for i in range(u)]
    for k in range(m):
        s_perm[rep[k]] = left[m - 1 - k]
    return a_perm, s_perm


def check_properties(a, s, a_perm, s_perm, beta: int, gamma: int) -> None:
    """What the lookup argument needs of a successful result."""
    assert sorted(a_perm) == sorted(a) and sorted(s_perm) == sorted(s)
    assert a_perm == sorted(a_perm)
    for i in range(len(a)):
        assert a_perm[i] == s_perm[i] or (i > 0 and a_perm[i] == a_perm[i - 1])
    lhs = rhs = 1
    for i in range(len(a)):
        lhs = lhs * (a[i] + beta) % R * (s[i] + gamma) % R
        rhs = rhs * (a_perm[i] + beta) % R * (s_perm[i] + gamma) % R
    assert lhs == rhs
