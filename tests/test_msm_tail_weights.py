"""The weights of the MSM reduction tail, against the CPU oracle.

Bucket b of a window lies in chunk c = b // CHUNK, and c = LO * hi + lo picks
its row and column in the window's grid of chunk totals. The tail weights
the bucket by (b % CHUNK + 1) inside its chunk, its column sum by lo, its row
sum by hi, and the host folds the three with CHUNK and CHUNK * LO. A wrong
weight anywhere shows as a wrong multiple of the base point, so the inputs
walk one entry over the edges of that decomposition, fill every bucket of a
window, and make sums inside the tail meet themselves or their negatives."""
import pytest

from spectre_amd import ffi

CHUNK, LO, HI = ffi.MSM_TAIL_CHUNK, ffi.MSM_TAIL_LO, ffi.MSM_TAIL_HI
WBITS = ffi.WINDOW_BITS

EDGE_DIGITS = [1, 2, CHUNK, CHUNK + 1, CHUNK * LO, CHUNK * LO + 1,
               CHUNK * LO * (HI - 1) + 1, 32767, 32768,
               0x8001, 0xffff]  # the last two recode negative and carry
SINGLE = ([(d, w) for w in (0, 7, 14) for d in EDGE_DIGITS] +
          [(d, 15) for d in (1, 0x3063)])  # top window: below the Fr modulus


def _sc(k: int) -> bytes:
    return k.to_bytes(32, "little")


@pytest.fixture(scope="module")
def inputs(oracle):
    """32768 random bases (and scalars for the random cases), made once."""
    return oracle.gen_msm_inputs(32768, 9500, fast=True)


@pytest.fixture(scope="module")
def base_p(inputs):
    return inputs[1][:64]


@pytest.mark.gpu
@pytest.mark.parametrize("d,w", SINGLE)
def test_single_entry(gpu, oracle, base_p, d, w):
    sc = _sc(d << (WBITS * w))
    assert gpu.msm(base_p, sc, 1) == oracle.msm(base_p, sc, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [0, 14])
def test_every_bucket_of_a_window(gpu, oracle, inputs, w):
    n = 32768
    bs = inputs[1]
    sc = b"".join(_sc((i + 1) << (WBITS * w)) for i in range(n))
    assert gpu.msm(bs, sc, n) == oracle.msm(bs, sc, n)


@pytest.mark.gpu
def test_equal_points_double_inside_the_tail(gpu, oracle, base_p):
    """Every bucket 0..4095 holds P: chunk totals, row sums, column sums and
    tree partners repeat, so adds meet equal operands and must double."""
    n = 4096
    sc = b"".join(_sc(i + 1) for i in range(n))
    assert gpu.msm(base_p * n, sc, n) == oracle.msm(base_p * n, sc, n)


@pytest.mark.gpu
def test_chunk_totals_cancel_weighted_sums_do_not(gpu, oracle, base_p):
    """P and -P alternate over neighbouring buckets: every T_c is the
    identity while every W_c is not."""
    n = 4096
    neg = oracle.g1_neg(base_p)
    bs = (base_p + neg) * (n // 2)
    sc = b"".join(_sc(i + 1) for i in range(n))
    assert gpu.msm(bs, sc, n) == oracle.msm(bs, sc, n)


@pytest.mark.gpu
def test_whole_rows_cancel(gpu, oracle, base_p):
    """Rows 1 and 3 of the chunk grid hold P in their first half and -P in
    their second: their row sums are the identity, their chunk totals and
    the column sums are not. Row 2 holds P throughout."""
    row = CHUNK * LO  # buckets per row
    neg = oracle.g1_neg(base_p)
    bs, sc = [], []
    for r in (1, 2, 3):
        for j in range(row):
            bs.append(neg if r != 2 and j >= row // 2 else base_p)
            sc.append(_sc(r * row + j + 1))
    n = len(bs)
    bs, sc = b"".join(bs), b"".join(sc)
    assert gpu.msm(bs, sc, n) == oracle.msm(bs, sc, n)


@pytest.fixture(scope="module")
def random300(oracle, inputs):
    n = 300
    sc, bs = inputs[0][:32 * n], inputs[1][:64 * n]
    return n, sc, bs, oracle.msm(bs, sc, n)


@pytest.mark.gpu
def test_random_300(gpu, random300):
    n, sc, bs, want = random300
    assert gpu.msm(bs, sc, n) == want


@pytest.fixture
def resident300(gpu, random300):
    n, sc, bs, _ = random300
    d_b, d_s = gpu.malloc(64 * n), gpu.malloc(32 * n)
    gpu.upload(d_b, bs)
    gpu.upload(d_s, sc)
    yield d_b, d_s
    gpu.free(d_b)
    gpu.free(d_s)


@pytest.mark.gpu
@pytest.mark.parametrize("w_cnt", [1, 4])
def test_window_shards(gpu, random300, resident300, w_cnt):
    n, _, _, want = random300
    d_b, d_s = resident300
    world = ffi.NUM_WINDOWS // w_cnt
    blob = b"".join(
        gpu.msm_shard_windows_device(d_b, d_s, n, r * w_cnt, w_cnt)
        for r in range(world))
    assert ffi.combine_window_partials(blob, world) == want


@pytest.mark.gpu
@pytest.mark.parametrize("nbatch", [2, 3])
def test_batches(gpu, oracle, inputs, nbatch):
    n = 300
    bs = inputs[1][:64 * n]
    vecs = [inputs[0][32 * n * b:32 * n * (b + 1)] for b in range(nbatch)]
    want = [oracle.msm(bs, v, n) for v in vecs]
    assert gpu.msm_batch(bs, b"".join(vecs), nbatch, n) == want


@pytest.mark.gpu
def test_three_calls_in_flight(gpu, random300, resident300):
    n, _, _, want = random300
    d_b, d_s = resident300
    pend = [gpu.msm_shard_device_async(d_b, d_s, n) for _ in range(3)]
    assert sorted(slot for _, slot in pend) == [0, 1, 2]
    try:
        for buf, slot in pend:
            gpu.msm_slot_wait(slot)
            assert ffi.combine_window_partials(bytes(buf), 1) == want
    finally:
        for _, slot in pend:
            gpu.msm_slot_wait(slot)
