"""The limb identity behind ff_sqr_cols (spectre_amd/csrc/ff.hpp), in plain
Python integers, no library and no GPU.

With B = 2^32 and limbs a_0..a_7 of a < 2^255,

    a^2 = sum_i a_i^2 B^(2i) + sum_{i<j} a_i D(i,j) B^(i+j)
    D(i,j)   = (a_j << 1 | a_(j-1) >> 31) mod B   for j > i + 1
    D(i,i+1) = (a_(i+1) << 1) mod B

which takes 36 limb products instead of 64. The identity drops bit 255 of
the doubled value, so it is false at 2^256 - 1: the documented precondition,
pinned in ff.hpp by a static_assert on the modulus.
"""
import random

import chain_operands as co
import edge_operands as eo

B = 1 << 32


def limbs(a: int) -> list:
    return [(a >> 32 * i) & (B - 1) for i in range(8)]


def column_products(a: int) -> list:
    """Column K -> the (x, y) limb products ff_sqr_cols adds to it."""
    l = limbs(a)
    adj = [0] + [(l[j] << 1) % B for j in range(1, 8)]
    dbl = [0] + [((l[j] << 1) | (l[j - 1] >> 31)) % B for j in range(1, 8)]
    cols = [[] for _ in range(15)]
    for k in range(15):
        i = max(0, k - 7)
        while 2 * i + 1 < k:
            cols[k].append((l[i], dbl[k - i]))
            i += 1
        if k % 2:
            cols[k].append((l[k // 2], adj[k // 2 + 1]))
        else:
            cols[k].append((l[k // 2], l[k // 2]))
    return cols


def sqr_by_identity(a: int) -> int:
    return sum(x * y << 32 * k
               for k, col in enumerate(column_products(a)) for x, y in col)


def test_product_count_and_column_height():
    cols = column_products(eo.ALL_ONES_LOW)
    assert sum(len(c) for c in cols) == 36
    # with the up to 8 m_k products of the reduction a column stays within
    # the 16 the (acc, ovf) scheme was sized for
    assert max(len(c) for c in cols) + 8 <= 16


def test_identity_at_the_edge_operands():
    for m in (eo.P, eo.R):
        for a in co.sqr_operands(m) + eo.specials(m):
            assert a < 1 << 255
            assert sqr_by_identity(a) == a * a, eo.hx(a)


def test_identity_at_random_operands():
    rng = random.Random(0x5a12)
    for _ in range(4000):
        a = rng.randrange(1 << 254)
        assert sqr_by_identity(a) == a * a, eo.hx(a)
    # and right up to the precondition's edge
    for a in ((1 << 255) - 1, (1 << 255) - 2, 1 << 254, (1 << 254) + 1):
        assert sqr_by_identity(a) == a * a, eo.hx(a)


def test_identity_needs_a_below_2_to_255():
    for a in ((1 << 256) - 1, (1 << 255) + 1, 1 << 255 | eo.ALL_ONES_LOW):
        assert sqr_by_identity(a) != a * a, eo.hx(a)
    # both moduli, and so every reduced element, are below the bound
    assert eo.R < eo.P < 1 << 255
