"""Whole MSMs through the XYZZ kernels (bucket accumulate, fix, chunk sums,
window tail and its one conversion to Jacobian) against the CPU oracle, at
n = 2^10 and 2^12 with the entries per accumulate thread forced to 4, 8 and 64.

The inputs aim at what the coordinates change: bases that repeat inside one
bucket in the orders [P, P, 2P] (a run doubles at ZZ == 1, then at ZZ != 1)
and [P, -P, Q] (a run passes through the identity and goes on), with scalars
equal over blocks of 48 entries so the repeats share buckets; all scalars
equal (one bucket per window and a run that spans every thread, so the fix
kernel adds XYZZ partials); scalars 1..3 (almost every bucket, and every
window but the first, is the identity in the chunk and tail kernels); a batch
of two; and two window shards combined on the host.
"""
import pytest

import edge_operands as eo

ref = eo.ref
E_VALUES = [4, 8, 64]
SIZES = [1 << 10, 1 << 12]
BLOCK = 48  # entries that share a scalar: whole [., ., .] patterns


def _patterned(bs, n, pattern):
    """n bases: for every third base P (and the next, Q) of bs, the three
    points pattern(P, Q)."""
    out = []
    for i in range(0, n, 3):
        p = ref.g1_from_bytes(bs[64 * i:64 * i + 64])
        q = ref.g1_from_bytes(bs[64 * (i + 1):64 * (i + 1) + 64])
        out += [ref.g1_to_bytes(x) for x in pattern(p, q)]
    return b"".join(out[:n])


def _blocked(sc, n):
    return b"".join(sc[32 * (i // BLOCK):32 * (i // BLOCK) + 32]
                    for i in range(n))


@pytest.fixture(scope="module")
def cases(oracle):
    """(name, bases, scalars, n, want); references computed once and shared
    by every E."""
    out = []
    for n in SIZES:
        sc, bs = oracle.gen_msm_inputs(n + 2, 9500 + n, fast=True)
        # one P per block, so a bucket holds P, P, 2P, P, P, 2P, ...
        rep = b"".join(bs[64 * (i // BLOCK):64 * (i // BLOCK) + 64]
                       for i in range(n + 2))
        inputs = [
            ("P-P-2P", _patterned(rep, n, lambda p, q: (p, p, ref.g1_add(p, p))),
             _blocked(sc, n)),
            ("P-negP-Q", _patterned(bs, n, lambda p, q: (p, ref.g1_neg(p), q)),
             _blocked(sc, n)),
            ("equal-scalars", bs[:64 * n], sc[:32] * n),
            ("sparse", bs[:64 * n],
             b"".join((1 + i % 3).to_bytes(32, "little") for i in range(n))),
        ]
        for name, b, s in inputs:
            out.append((f"{name}-n{n}", b, s, n, oracle.msm(b, s, n)))
    return out


@pytest.fixture(scope="module")
def batch_cases(oracle, cases):
    """(bases, two scalar vectors, n, [want, want]): the P-P-2P bases under
    their blocked scalars and under one scalar for all."""
    out = []
    for name, bs, sc, n, want in cases:
        if name.startswith("P-P-2P"):
            eq = sc[:32] * n
            out.append((bs, sc + eq, n, [want, oracle.msm(bs, eq, n)]))
    return out


@pytest.fixture
def set_e(gpu):
    yield gpu.set_msm_acc_entries
    gpu.set_msm_acc_entries(0)


@pytest.mark.gpu
@pytest.mark.parametrize("e", E_VALUES)
def test_msm_runs_match_oracle(gpu, cases, set_e, e):
    set_e(e)
    for name, bs, sc, n, want in cases:
        assert gpu.msm(bs, sc, n, canonical=True) == want, (e, name)


@pytest.mark.gpu
@pytest.mark.parametrize("e", E_VALUES)
def test_msm_runs_batch_of_two(gpu, batch_cases, set_e, e):
    set_e(e)
    assert len(batch_cases) == len(SIZES)
    for bs, sc, n, want in batch_cases:
        assert gpu.msm_batch(bs, sc, 2, n) == want, (e, n)


@pytest.mark.gpu
@pytest.mark.parametrize("e", E_VALUES)
def test_msm_runs_two_window_shards(gpu, cases, set_e, e):
    from spectre_amd import ffi
    set_e(e)
    for name, bs, sc, n, want in cases:
        if n != SIZES[0]:
            continue
        d_b, d_s = gpu.malloc(64 * n), gpu.malloc(32 * n)
        try:
            gpu.upload(d_b, bs)
            gpu.upload(d_s, sc)
            half = ffi.NUM_WINDOWS // 2
            blob = b"".join(
                gpu.msm_shard_windows_device(d_b, d_s, n, r * half, half)
                for r in range(2))
            assert ffi.combine_window_partials(blob, 2) == want, (e, name)
        finally:
            gpu.free(d_b)
            gpu.free(d_s)
