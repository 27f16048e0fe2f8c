"""Operands aimed at the carry-chain add / sub / reduce and at the column
squaring of ff.hpp.

TEST INFRASTRUCTURE, shared by test_field_chain_edges.py and
test_sqr_limb_identity.py. Like tests/edge_operands.py everything is a
Montgomery *image*: an integer x with 0 <= x < m, the eight limbs a kernel
sees. Computed once per process; users leave it unchanged.
"""
import functools
import random

import edge_operands as eo

TOP_BELOW = 0x30644e71  # one below the top limb of both moduli


def _anchors(m: int) -> list:
    rng = random.Random(0xc4a1 + m % 65537)
    return [0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2, 1 << 128,
            (1 << 224) - 1, eo.ALL_ONES_LOW, eo.MONT % m] + \
           [rng.randrange(m) for _ in range(8)]


@functools.lru_cache(maxsize=None)
def boundary_pairs(m: int) -> tuple:
    """Pairs with a + b in {m-1, m, m+1} and pairs with a - b in {-1, 0, 1}:
    the sums and differences on either side of the reduction's decision."""
    out = []
    for a in _anchors(m):
        for t in (m - 1, m, m + 1):
            if 0 <= t - a < m:
                out.append((a, t - a))
        for d in (-1, 0, 1):
            if 0 <= a - d < m:
                out.append((a, a - d))
    assert {(a + b) - m for a, b in out} >= {-1, 0, 1}
    assert {a - b for a, b in out} >= {-1, 0, 1}
    return tuple(out)


@functools.lru_cache(maxsize=None)
def ripple_pairs(m: int) -> tuple:
    """A carry (add) or a borrow (sub) that runs through k whole limbs,
    k = 1..7, and the two ends: (0, 1) and (m-1, m-1)."""
    out = [(0, 1), (m - 1, m - 1)]
    for k in range(1, 8):
        out += [((1 << 32 * k) - 1, 1), (1 << 32 * k, 1)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def alternating65(m: int, op: str) -> tuple:
    """65 pairs, one wave and a lane. Even elements take the correction of
    `op` (sub: a < b, the chain borrows; add: a + b >= m, the trial subtract
    is kept), odd elements do not, so neighbouring lanes always differ."""
    rng = random.Random(0xa17e + m % 65537 + (op == "add"))
    out = []
    for i in range(65):
        while True:
            a, b = rng.randrange(m), rng.randrange(m)
            corrected = a < b if op == "sub" else a + b >= m
            if corrected == (i % 2 == 0):
                break
        out.append((a, b))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sqr_operands(m: int) -> tuple:
    """Images that stress the doubled limbs of the column squaring: bit 31 of
    one limb j (it moves into limb j+1's doubled value; j = 7 would be 2^255,
    which is no reduced element), bit 31 of all of limbs 0..6 under two top
    limbs, and the large reduced values."""
    bits31 = sum(1 << (32 * j + 31) for j in range(7))
    xs = [1 << (32 * j + 31) for j in range(7)]
    xs += [bits31, bits31 | (TOP_BELOW << 224), eo.ALL_ONES_LOW, m - 1,
           (m - 1) // 2, (m + 1) // 2, 1 << 253, ((1 << 254) - 1) % m]
    assert all(0 <= x < m for x in xs) and len(set(xs)) == len(xs)
    return tuple(xs)
