"""Bucket accumulation under every partition: the entries-per-thread value E
only decides which thread adds which sorted entry, so the affine result must
be byte-identical to the CPU oracle for any E and for the auto choice.

The inputs aim at the partition's edges: fewer entries than one thread's
range, entry counts that are no multiple of E or of the 4-entry load, a short
last range, one bucket spanning many threads (the k_bucket_fix merge), the
doubling and cancel-to-infinity paths inside a run, and digits that carry
through every window to the skip sentinel.
"""
import pytest

E_VALUES = [4, 8, 12, 64, 4096, 0]  # 0 = auto
SIZES = [1, 3, 5, 63, 64, 65, 257, 1000, 4096]

# canonical scalars below the Fr modulus (top 16-bit digit < 0x3064)
S_ALL_FFFF = b"\xff\xff" * 15 + b"\xff\x2f"
S_ALL_8000 = b"\x00\x80" * 15 + b"\x00\x20"
S_ONE = (1).to_bytes(32, "little")
S_ZERO = bytes(32)


def _mont(oracle, sc, n):
    return b"".join(oracle.fr_from_canonical(sc[32 * i:32 * i + 32])
                    for i in range(n))


@pytest.fixture(scope="module")
def cases(oracle):
    """(name, bases, scalars, n, canonical, want) — references computed once
    and shared by every E."""
    out = []

    def add(name, bs, sc, n):
        out.append((name, bs, sc, n, True, oracle.msm(bs, sc, n)))

    for idx, n in enumerate(SIZES):
        sc, bs = oracle.gen_msm_inputs(n, 9100 + idx, fast=True)
        add(f"n{n}", bs, sc, n)
        out.append((f"n{n}-mont", bs, _mont(oracle, sc, n), n, False,
                    out[-1][5]))

    n = 1000
    sc, bs = oracle.gen_msm_inputs(n, 9200, fast=True)
    add("equal-scalars", bs, sc[:32] * n, n)  # one bucket per window
    add("zero-scalars", bs, S_ZERO * n, n)    # no real entry at all
    add("one-scalars", bs, S_ONE * n, n)
    add("digits-ffff", bs, S_ALL_FFFF * n, n)
    add("digits-8000", bs, S_ALL_8000 * n, n)
    add("digits-mixed", bs[:64 * 300],
        (S_ALL_FFFF + S_ALL_8000 + sc[:32]) * 100, 300)

    p, q = bs[:64], bs[64:128]
    s = sc[:32]
    add("same-point", p * 5, s * 5, 5)  # P+P doubles inside the run
    add("same-point-long", p * 257, s * 257, 257)
    # P, -P cancel to infinity mid-run; the run goes on with Q, P, -P, Q...
    cancel = (p + oracle.g1_neg(p) + q) * 7
    add("cancel", cancel, s * 21, 21)
    return out


@pytest.fixture
def set_e(gpu):
    yield gpu.set_msm_acc_entries
    gpu.set_msm_acc_entries(0)


@pytest.mark.gpu
@pytest.mark.parametrize("e", E_VALUES)
def test_msm_any_partition_matches_oracle(gpu, cases, set_e, e):
    set_e(e)
    for name, bs, sc, n, canonical, want in cases:
        got = gpu.msm(bs, sc, n, canonical=canonical)
        assert got == want, (e, name)


@pytest.mark.gpu
@pytest.mark.parametrize("e", E_VALUES)
def test_msm_window_sharded_any_partition(gpu, oracle, set_e, e):
    from spectre_amd import ffi
    n = 300
    sc, bs = oracle.gen_msm_inputs(n, 9300, fast=True)
    want = oracle.msm(bs, sc, n)
    d_b = gpu.malloc(64 * n)
    d_s = gpu.malloc(32 * n)
    gpu.upload(d_b, bs)
    gpu.upload(d_s, sc)
    try:
        set_e(e)
        for w_cnt in (1, 4):
            world = ffi.NUM_WINDOWS // w_cnt
            blob = b"".join(
                gpu.msm_shard_windows_device(d_b, d_s, n, r * w_cnt, w_cnt)
                for r in range(world))
            assert ffi.combine_window_partials(blob, world) == want, (e, w_cnt)
    finally:
        gpu.free(d_b)
        gpu.free(d_s)


@pytest.mark.gpu
@pytest.mark.parametrize("e", E_VALUES)
def test_msm_batch_any_partition(gpu, oracle, set_e, e):
    n = 300
    sc0, bs = oracle.gen_msm_inputs(n, 9400, fast=True)
    sc1, _ = oracle.gen_msm_inputs(n, 9401, fast=True)
    want = [oracle.msm(bs, sc0, n), oracle.msm(bs, sc1, n)]
    set_e(e)
    assert gpu.msm_batch(bs, sc0 + sc1, 2, n) == want, e


@pytest.mark.gpu
def test_set_msm_acc_entries_rejects_non_quads(gpu):
    for bad in (1, 2, 6, 63):
        with pytest.raises(RuntimeError):
            gpu.set_msm_acc_entries(bad)
    gpu.set_msm_acc_entries(0)


def test_auto_entries_rule():
    """The auto rule (host-only, no GPU): E is a multiple of 4 inside its
    clamp; large inputs get the maximum, tiny ones the minimum, and between
    the two the grid is the targeted number of blocks per CU and no more.
    Fill bound: there E is the exact share (> E_MIN = 8) rounded up to an
    integer and then to a multiple of 4, less than 4 more, so more than
    8/12 of the targeted threads have a range; 0.6 leaves room for the
    last partial block."""
    from spectre_amd import ffi
    lo, hi, thr = ffi.MSM_ACC_E_MIN, ffi.MSM_ACC_E_MAX, ffi.MSM_ACC_THREADS
    inputs = [
        ((1 << 20) * 16, 256, 3),  # the benchmark shape, 3 resident blocks
        ((1 << 20) * 16, 256, 4),
        ((1 << 23) * 16, 256, 3),
        ((1 << 32) - 1, 256, 3),
        ((1 << 19) * 16, 256, 3),  # exactly the targeted grid at E_MAX
        ((1 << 19) * 16 - 1, 256, 3),
        ((1 << 18) * 16, 256, 3), ((1 << 17) * 16 + 5, 256, 3),
        ((1 << 16) * 16, 256, 3), ((1 << 16) * 16, 256, 1),
        (131072 * 8 + 1, 256, 3),  # just above the targeted grid at E_MIN
        (16, 256, 3), (0, 256, 3), (300 * 16, 304, 2), ((1 << 16) * 16, 64, 1),
    ]
    for entries, cus, resident in inputs:
        e = ffi.msm_acc_auto_entries(entries, cus, resident)
        assert e % 4 == 0 and lo <= e <= hi, (entries, cus, resident, e)
        target = cus * min(resident, ffi.MSM_ACC_TARGET_BLOCKS)
        if entries >= target * thr * hi:
            assert e == hi, (entries, cus, resident, e)
        elif entries <= target * thr * lo:
            assert e == lo, (entries, cus, resident, e)
        else:
            blocks = -(-(-(-entries // e)) // thr)
            assert 0.6 * target <= blocks <= target, (entries, cus, resident, e)
    assert ffi.msm_acc_auto_entries((1 << 20) * 16, 256, 3) == 64
    assert ffi.msm_acc_auto_entries((1 << 20) * 16, 256, 4) == 64
    assert ffi.msm_acc_auto_entries((1 << 16) * 16, 256, 3) == 8
