"""The index identity behind the extend pass of ntt.hip, in plain Python
integers over tests/golden/bn254_ref.py's modulus. CPU only.

A tile of length L whose elements from L' = L >> p up are zero goes through
the first p levels of the in-place DIF as a copy and one multiply per level,
so after them block q (q < 2^p) of the tile holds, at offset j < L',
x[j] * root^(j * bitrev(q, p)). The kernel's load phase writes that directly
and starts the butterflies at level p; here the textbook DIF over the padded
tile and that pruned form must agree position by position."""
import importlib.util
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "bn254_ref", os.path.join(HERE, "golden", "bn254_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
R = ref.R


def bitrev(x: int, bits: int) -> int:
    out = 0
    for _ in range(bits):
        out = out << 1 | x & 1
        x >>= 1
    return out


def dif(a, root: int, log_l: int, start: int = 0):
    """The in-place DIF of lds_dif from level `start` on: level k pairs
    (i0, i0 + h) with h = L/2 >> k and twiddle root^(j * (L/2)/h); output
    index bitrev(s) ends at position s."""
    a = list(a)
    size = 1 << log_l
    for level in range(start, log_l):
        h = size >> 1 >> level
        stride = (size >> 1) // h
        for blk in range(size // (2 * h)):
            for j in range(h):
                i0, i1 = blk * 2 * h + j, blk * 2 * h + j + h
                u, v = a[i0], a[i1]
                a[i0] = (u + v) % R
                a[i1] = (u - v) * pow(root, j * stride, R) % R
    return a


def pruned(x, root: int, log_l: int, p: int):
    """Replicate x (L' elements) into the 2^p blocks with the multiplier
    root^(j * bitrev(q, p)), exponent reduced through root^(L/2) = -1 the way
    the kernel reads its half-length twiddle table, then DIF from level p."""
    size = 1 << log_l
    lp, half = size >> p, size >> 1
    tile = [None] * size
    for j in range(lp):
        for q in range(1 << p):
            e = j * bitrev(q, p)
            assert e < size
            t = x[j] * pow(root, e & (half - 1), R) % R
            tile[q * lp + j] = (R - t) % R if e & half else t
    assert None not in tile
    return dif(tile, root, log_l, start=p)


def test_dif_is_the_dft_in_bit_reversed_order():
    rng = random.Random(2201)
    for log_l in range(1, 5):
        size = 1 << log_l
        root = ref.fr_root_of_unity(log_l)
        x = [rng.randrange(R) for _ in range(size)]
        got = dif(x, root, log_l)
        for s in range(size):
            t = bitrev(s, log_l)
            assert got[s] == sum(x[i] * pow(root, i * t, R)
                                 for i in range(size)) % R


def test_pruned_levels_equal_full_dif_on_padded_tile():
    rng = random.Random(2202)
    for log_l in range(1, 7):           # L = 2 .. 64
        size = 1 << log_l
        root = ref.fr_root_of_unity(log_l)
        for p in range(log_l + 1):      # every p with 2^p <= L; L' down to 1
            lp = size >> p
            x = [rng.randrange(R) for _ in range(lp)]
            full = dif(x + [0] * (size - lp), root, log_l)
            assert pruned(x, root, log_l, p) == full, (size, p)


def test_pruned_levels_with_zero_and_unit_inputs():
    """Zeros inside the loaded part (a first axis shorter than ext_bits loads
    zeros below L' too) and x = 1, where every block is the bare twiddle."""
    for log_l, p in ((3, 1), (4, 4), (6, 2)):
        size = 1 << log_l
        root = ref.fr_root_of_unity(log_l)
        lp = size >> p
        for x in ([0] * lp, [1] * lp, [1] + [0] * (lp - 1)):
            full = dif(x + [0] * (size - lp), root, log_l)
            assert pruned(x, root, log_l, p) == full, (size, p, x)
