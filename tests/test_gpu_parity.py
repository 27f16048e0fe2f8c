"""GPU parity tests (@gpu): the HIP path vs the CPU oracle and the committed
golden vectors, bit-exact, including the BASELINE-size property checks."""
import hashlib

import pytest

pytestmark = pytest.mark.gpu


def hx(s):
    return bytes.fromhex(s)


def _omega(log_n, oracle, golden):
    for c in golden("ntt.json")["seeded_cases"]:
        if c["log_n"] == 12:
            w = hx(c["omega_mont"])
    if log_n > 12:  # lift via the 2^28 root: omega_28^(2^(28-log_n))
        w = ROOT28
        for _ in range(28 - log_n):
            w = oracle.fr_mul(w, w)
    else:
        for _ in range(12 - log_n):
            w = oracle.fr_mul(w, w)
    return w


# 2^28 primitive root of BN254 Fr, Montgomery form (= 7^((r-1)/2^28));
# verified against the committed 2^12 fixture root in test_root_consistency.
ROOT28 = None


@pytest.fixture(scope="module", autouse=True)
def _root28(oracle):
    global ROOT28
    # GENERATOR=7 canonical -> mont; exponent (r-1)/2^28
    r = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    g7 = oracle.fr_from_canonical((7).to_bytes(32, "little"))
    e = ((r - 1) >> 28).to_bytes(32, "little")
    ROOT28 = oracle.fr_pow(g7, e)
    yield


def test_root_consistency(oracle, golden):
    w = ROOT28
    for _ in range(28 - 12):
        w = oracle.fr_mul(w, w)
    for c in golden("ntt.json")["seeded_cases"]:
        if c["log_n"] == 12:
            assert w.hex() == c["omega_mont"]


# ---------------------------------------------------------------- MSM
def test_msm_inline_golden(gpu, golden):
    for i, c in enumerate(golden("msm.json")["inline_cases"]):
        n = c["n"]
        if n == 0:
            continue  # host-pointer path handles n=0 below
        sc = b"".join(hx(s) for s in c["scalars_canon"])
        scm = b"".join(hx(s) for s in c["scalars_mont"])
        bs = b"".join(hx(s) for s in c["bases"])
        assert gpu.msm(bs, sc, n, canonical=True).hex() == c["result"], i
        assert gpu.msm(bs, scm, n, canonical=False).hex() == c["result"], i


def test_msm_n0(gpu):
    assert gpu.msm(b"", b"", 0) == bytes(64)


def test_msm_seeded_golden(gpu, oracle, golden):
    for c in golden("msm.json")["seeded_cases"]:
        sc, bs = oracle.gen_msm_inputs(c["n"], c["seed"])
        assert gpu.msm(bs, sc, c["n"]).hex() == c["result"], c["n"]


@pytest.mark.parametrize("log_n", [12, 16])
def test_msm_vs_oracle(gpu, oracle, log_n):
    n = 1 << log_n
    sc, bs = oracle.gen_msm_inputs(n, 9000 + log_n, fast=True)
    want = oracle.msm(bs, sc, n)
    assert gpu.msm(bs, sc, n) == want


def test_msm_2pow20_vs_oracle(gpu, oracle):
    """Full BASELINE config[1] size, exact parity."""
    n = 1 << 20
    sc, bs = oracle.gen_msm_inputs(n, 42, fast=True)
    want = oracle.msm(bs, sc, n)
    assert gpu.msm(bs, sc, n) == want


@pytest.mark.parametrize("log_n", [22, 23])
def test_msm_aggregation_sizes_vs_oracle(gpu, oracle, log_n):
    """Aggregation-circuit MSM sizes (K=23/24 proofs commit at 2^23/2^24;
    2^22 covers the k=20 extended-domain h commits)."""
    n = 1 << log_n
    sc, bs = oracle.gen_msm_inputs(n, 2200 + log_n, fast=True)
    want = oracle.msm(bs, sc, n)
    assert gpu.msm(bs, sc, n) == want


def test_msm_bases_cache(gpu, oracle):
    n = 4096
    sc, bs = oracle.gen_msm_inputs(n, 31, fast=True)
    r1 = gpu.msm(bs, sc, n, bases_id=77)
    r2 = gpu.msm(None, sc, n, bases_id=77)  # cached upload
    assert r1 == r2 == oracle.msm(bs, sc, n)


def test_msm_async_pipeline_matches_sync(gpu, oracle):
    """Depth-2 pipelined MSMs on the two per-device slots: every in-flight
    call returns exactly the synchronous result, including when two
    different inputs are in flight on the two slots at once."""
    from spectre_amd import ffi
    n = 1 << 14
    sc_a, bs = oracle.gen_msm_inputs(n, 61, fast=True)
    sc_b = oracle.gen_msm_inputs(n, 62, fast=True)[0]
    d_b = gpu.malloc(64 * n)
    d_sa = gpu.malloc(32 * n)
    d_sb = gpu.malloc(32 * n)
    gpu.upload(d_b, bs)
    gpu.upload(d_sa, sc_a)
    gpu.upload(d_sb, sc_b)
    want_a = ffi.combine_partials(gpu.msm_shard_device(d_b, d_sa, n), 1)
    want_b = ffi.combine_partials(gpu.msm_shard_device(d_b, d_sb, n), 1)
    # interleave: a,b,a,b,... with both slots busy simultaneously
    pend = []
    got = []
    for i in range(6):
        buf, slot = gpu.msm_shard_device_async(d_b, d_sa if i % 2 == 0 else d_sb, n)
        pend.append((buf, slot))
        if len(pend) == 2:
            b0, s0 = pend.pop(0)
            gpu.msm_slot_wait(s0)
            got.append(ffi.combine_partials(bytes(b0), 1))
    for b0, s0 in pend:
        gpu.msm_slot_wait(s0)
        got.append(ffi.combine_partials(bytes(b0), 1))
    for i, g in enumerate(got):
        assert g == (want_a if i % 2 == 0 else want_b), f"call {i}"
    for p in (d_b, d_sa, d_sb):
        gpu.free(p)


def test_msm_two_device_in_library(oracle):
    """In-library multi-device sharding (spectre_gpu_msm_g1 num_gpus=2) must
    equal the single-device result bit-for-bit. Skips on 1-GPU boxes (the
    per-round driver box); armed for the 8-GPU scaling node (VERDICT r01
    item 9: keep the 8-GPU path warm)."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 devices")
    from spectre_amd import SpectreGpu
    g = SpectreGpu([0, 1])
    try:
        n = 1 << 14
        sc, bs = oracle.gen_msm_inputs(n, 63, fast=True)
        one = g.msm(bs, sc, n, num_gpus=1)
        two = g.msm(bs, sc, n, num_gpus=2)
        assert one == two
        assert one == oracle.msm(bs, sc, n)
    finally:
        g.close()


def test_msm_window_shard_combine_matches_direct(gpu, oracle):
    """Window-sharded shards (disjoint window ranges over ALL points,
    concatenated in rank order) must equal the direct result bit-for-bit —
    the default N>1 exchange (pure allgather, no reduction)."""
    from spectre_amd import ffi
    n = 1 << 13
    sc, bs = oracle.gen_msm_inputs(n, 64, fast=True)
    direct = gpu.msm(bs, sc, n)
    d_b = gpu.malloc(64 * n)
    d_s = gpu.malloc(32 * n)
    gpu.upload(d_b, bs)
    gpu.upload(d_s, sc)
    for world in (2, 4, 8):
        w_cnt = ffi.NUM_WINDOWS // world
        blob = b"".join(
            gpu.msm_shard_windows_device(d_b, d_s, n, r * w_cnt, w_cnt)
            for r in range(world))
        assert ffi.combine_window_partials(blob, world) == direct, world
    # async variant, interleaved across two ranks' window sets
    w_cnt = ffi.NUM_WINDOWS // 2
    b0, s0 = gpu.msm_shard_windows_device_async(d_b, d_s, n, 0, w_cnt)
    b1, s1 = gpu.msm_shard_windows_device_async(d_b, d_s, n, w_cnt, w_cnt)
    gpu.msm_slot_wait(s0)
    gpu.msm_slot_wait(s1)
    assert ffi.combine_window_partials(bytes(b0) + bytes(b1), 2) == direct
    gpu.free(d_b)
    gpu.free(d_s)


def test_msm_shard_combine_matches_direct(gpu, oracle):
    """Two shards on one device + host combine == unsharded result — the
    exact exchange the multi-GPU path performs (bit-identical by affine
    canonicality)."""
    from spectre_amd import ffi
    n = 1 << 13
    sc, bs = oracle.gen_msm_inputs(n, 60, fast=True)
    direct = gpu.msm(bs, sc, n)
    half = n // 2
    parts = b""
    d_b = gpu.malloc(64 * half)
    d_s = gpu.malloc(32 * half)
    for lo in (0, half):
        gpu.upload(d_b, bs[64 * lo:64 * (lo + half)])
        gpu.upload(d_s, sc[32 * lo:32 * (lo + half)])
        parts += gpu.msm_shard_device(d_b, d_s, half)
    gpu.free(d_b)
    gpu.free(d_s)
    assert ffi.combine_partials(parts, 2) == direct


def test_msm_batch_matches_individual(gpu, oracle):
    """Batched MSM (shared bases, fused pipeline) must equal per-vector
    results bit-for-bit."""
    n, nbatch = 2048, 5
    _, bs = oracle.gen_msm_inputs(n, 70, fast=True)
    scal = b""
    singles = []
    for b in range(nbatch):
        sc, _ = oracle.gen_msm_inputs(n, 71 + b, fast=True)
        scal += sc
        singles.append(oracle.msm(bs, sc, n))
    got = gpu.msm_batch(bs, scal, nbatch, n)
    assert got == singles
    # edge: batch with an all-zero vector and a duplicate vector
    scal2 = bytes(32 * n) + scal[:32 * n] + scal[:32 * n]
    got2 = gpu.msm_batch(bs, scal2, 3, n)
    assert got2[0] == bytes(64)
    assert got2[1] == got2[2] == singles[0]


def test_msm_device_resident(gpu, oracle):
    n = 4096
    sc, bs = oracle.gen_msm_inputs(n, 61, fast=True)
    d_b = gpu.malloc(64 * n)
    d_s = gpu.malloc(32 * n)
    gpu.upload(d_b, bs)
    gpu.upload(d_s, sc)
    got = gpu.msm_device(d_b, d_s, n)
    gpu.free(d_b)
    gpu.free(d_s)
    assert got == oracle.msm(bs, sc, n)


# ---------------------------------------------- scratch growth, slot hand-off
@pytest.fixture
def fresh_gpu():
    """A context of its own, so the scratch starts empty and no slot is busy."""
    from spectre_amd import SpectreGpu
    g = SpectreGpu([0])
    yield g
    g.close()


def _device_inputs(g, bs, sc):
    d_b = g.malloc(len(bs))
    d_s = g.malloc(len(sc))
    g.upload(d_b, bs)
    g.upload(d_s, sc)
    return d_b, d_s


def test_msm_scratch_regrowth_sequence(fresh_gpu, oracle):
    """Walks every MSM scratch group of one context through grow, reuse and
    grow again (entries, side arrays, buckets, sort temp, pinned sums, the
    host-pointer scalars/bases and the bases cache); every result bit-exact
    against the oracle."""
    from spectre_amd import ffi
    g = fresh_gpu

    def inputs(n, seed):
        sc, bs = oracle.gen_msm_inputs(n, seed, fast=True)
        return sc, bs, oracle.msm(bs, sc, n)

    small = inputs(64, 9101)
    big = inputs(4096, 9102)
    for n, (sc, bs, want) in ((64, small), (4096, big), (64, small)):
        assert g.msm(bs, sc, n) == want, n
    # batch: more windows' worth of buckets than any single call
    n = 257
    _, bs = oracle.gen_msm_inputs(n, 9103, fast=True)
    vecs = [oracle.gen_msm_inputs(n, 9104 + b, fast=True)[0] for b in range(3)]
    assert g.msm_batch(bs, b"".join(vecs), 3, n) == [
        oracle.msm(bs, sc, n) for sc in vecs]
    # 4 entries per thread: more accumulate threads, so larger side arrays,
    # than the auto choice (>= MSM_ACC_E_MIN) gave the same n above
    g.set_msm_acc_entries(4)
    sc, bs, want = big
    assert g.msm(bs, sc, 4096) == want
    g.set_msm_acc_entries(0)
    # window shards on the shrunk-again scratch, spliced into the full-range
    # shard's other windows (window sums are Jacobian: compare the affine)
    n = 1000
    sc, bs, want = inputs(n, 9110)
    d_b, d_s = _device_inputs(g, bs, sc)
    blob = bytearray(g.msm_shard_device(d_b, d_s, n))
    for w_lo in (4, 12):
        blob[96 * w_lo:96 * (w_lo + 4)] = g.msm_shard_windows_device(
            d_b, d_s, n, w_lo, 4)
    assert ffi.combine_window_partials(bytes(blob), 1) == want
    g.free(d_b)
    g.free(d_s)
    # cached bases: upload on the miss, no bases needed on the hit
    n = 300
    sc, bs, want = inputs(n, 9111)
    assert g.msm(bs, sc, n, bases_id=91) == want
    assert g.msm(None, sc, n, bases_id=91) == want


def test_ntt_scratch_regrowth_sequence(fresh_gpu, oracle, golden):
    """NTT io/tmp/coset scratch and the plan cache of one context: small,
    large, small again with a coset, large inverse with a coset."""
    g = fresh_gpu
    g5 = oracle.fr_from_canonical((5).to_bytes(32, "little"))
    for log_n, inverse, coset in ((4, False, None), (13, False, None),
                                  (4, False, g5), (13, True, g5)):
        a = oracle.gen_fr_vector(1 << log_n, 9200 + log_n)
        w = _omega(log_n, oracle, golden)
        if inverse:
            w = oracle.fr_inv(w)
        got = g.ntt(a, log_n, w, inverse=inverse, coset_gen=coset)
        assert got == oracle.ntt(a, log_n, w, inverse=inverse,
                                 coset_gen=coset), (log_n, inverse)


def _pipe_slots():
    import os
    return min(max(int(os.environ.get("SPECTRE_PIPE_SLOTS", "3")), 1), 3)


def test_msm_async_slot_exhaustion_is_loud(fresh_gpu, oracle):
    """Enqueueing without waiting wraps round to the busy slot 0 at attempt
    slots + 1: that call is rejected by return code (no kernel runs), every
    accepted call still delivers, and the context stays usable."""
    from spectre_amd import ffi
    g = fresh_gpu
    n = 257
    sc, bs = oracle.gen_msm_inputs(n, 9301, fast=True)
    want = oracle.msm(bs, sc, n)
    d_b, d_s = _device_inputs(g, bs, sc)
    sync_partials = g.msm_shard_device(d_b, d_s, n)
    assert ffi.combine_partials(sync_partials, 1) == want
    pend, rejected = [], []
    for attempt in range(1, 5):
        try:
            pend.append(g.msm_shard_device_async(d_b, d_s, n))
        except RuntimeError as e:
            assert "already has a call in flight" in str(e)
            rejected.append(attempt)
            break
    assert rejected == [_pipe_slots() + 1]
    assert [slot for _, slot in pend] == list(range(_pipe_slots()))
    for buf, slot in pend:
        g.msm_slot_wait(slot)
        assert ffi.combine_partials(bytes(buf), 1) == want, slot
    assert g.msm_shard_device(d_b, d_s, n) == sync_partials
    g.free(d_b)
    g.free(d_s)


def test_msm_sync_on_busy_slot_is_rejected(fresh_gpu, oracle):
    """A synchronous call shares slot 0 with the first async call: while that
    one is pending it must be rejected, not overwrite the pending window
    sums; after the wait both deliver."""
    from spectre_amd import ffi
    g = fresh_gpu
    n = 257
    sc, bs = oracle.gen_msm_inputs(n, 9302, fast=True)
    want = oracle.msm(bs, sc, n)
    d_b, d_s = _device_inputs(g, bs, sc)
    buf, slot = g.msm_shard_device_async(d_b, d_s, n)
    assert slot == 0
    with pytest.raises(RuntimeError, match="already has a call in flight"):
        g.msm_shard_device(d_b, d_s, n)
    g.msm_slot_wait(0)
    assert ffi.combine_partials(bytes(buf), 1) == want
    assert ffi.combine_partials(g.msm_shard_device(d_b, d_s, n), 1) == want
    g.free(d_b)
    g.free(d_s)


# ---------------------------------------------------------------- NTT
def test_ntt_inline_golden(gpu, golden):
    for c in golden("ntt.json")["inline_cases"]:
        ln = c["log_n"]
        inp = b"".join(hx(x) for x in c["input_mont"])
        om = hx(c["omega_mont"])
        assert gpu.ntt(inp, ln, om).hex() == "".join(c["ntt"]), (ln, "fwd")


def test_ntt_inline_golden_inverse_coset(gpu, oracle, golden):
    for c in golden("ntt.json")["inline_cases"]:
        ln = c["log_n"]
        inp = b"".join(hx(x) for x in c["input_mont"])
        om = hx(c["omega_mont"])
        out_i = gpu.ntt(inp, ln, oracle.fr_inv(om), inverse=True)
        assert out_i.hex() == "".join(c["intt"]), (ln, "inv")
        out_c = gpu.ntt(inp, ln, om, coset_gen=hx(c["coset_g_mont"]))
        assert out_c.hex() == "".join(c["coset_ntt"]), (ln, "coset")


def test_ntt_seeded_golden(gpu, oracle, golden):
    for c in golden("ntt.json")["seeded_cases"]:
        ln = c["log_n"]
        inp = oracle.gen_fr_vector(1 << ln, c["seed"])
        om = hx(c["omega_mont"])
        assert hashlib.sha256(gpu.ntt(inp, ln, om)).hexdigest() == c["ntt_sha256"]
        out_i = gpu.ntt(inp, ln, oracle.fr_inv(om), inverse=True)
        assert hashlib.sha256(out_i).hexdigest() == c["intt_sha256"]


@pytest.mark.parametrize("log_n", [13, 16, 18])
def test_ntt_vs_oracle(gpu, oracle, golden, log_n):
    """Two-pass GPU path vs oracle at sizes the oracle runs in seconds."""
    n = 1 << log_n
    a = oracle.gen_fr_vector(n, 100 + log_n)
    w = _omega(log_n, oracle, golden)
    assert gpu.ntt(a, log_n, w) == oracle.ntt(a, log_n, w)
    wi = oracle.fr_inv(w)
    assert gpu.ntt(a, log_n, wi, inverse=True) == oracle.ntt(a, log_n, wi,
                                                             inverse=True)


def test_ntt_coset_vs_oracle(gpu, oracle, golden):
    log_n = 14
    n = 1 << log_n
    a = oracle.gen_fr_vector(n, 777)
    w = _omega(log_n, oracle, golden)
    g = oracle.fr_from_canonical((5).to_bytes(32, "little"))
    assert gpu.ntt(a, log_n, w, coset_gen=g) == oracle.ntt(a, log_n, w,
                                                           coset_gen=g)
    gi = oracle.fr_inv(g)
    wi = oracle.fr_inv(w)
    assert (gpu.ntt(a, log_n, wi, inverse=True, coset_gen=gi)
            == oracle.ntt(a, log_n, wi, inverse=True, coset_gen=gi))


@pytest.mark.parametrize("log_n", [20, 23])
def test_ntt_roundtrip_full_size(gpu, oracle, golden, log_n):
    """BASELINE-size property check (oracle-free at this size):
    iNTT(NTT(a)) == a and coset round trip, device-resident."""
    n = 1 << log_n
    a = oracle.gen_fr_vector(n, 4000 + log_n)
    w = _omega(log_n, oracle, golden)
    wi = oracle.fr_inv(w)
    d = gpu.malloc(32 * n)
    gpu.upload(d, a)
    gpu.ntt_device(d, log_n, w)
    gpu.ntt_device(d, log_n, wi, inverse=True)
    assert gpu.download(d, 32 * n) == a
    g = oracle.fr_from_canonical((5).to_bytes(32, "little"))
    gpu.ntt_device(d, log_n, w, coset_gen=g)
    gpu.ntt_device(d, log_n, wi, inverse=True, coset_gen=oracle.fr_inv(g))
    assert gpu.download(d, 32 * n) == a
    gpu.free(d)


def test_ntt_full_size_spotcheck_vs_dft(gpu, oracle, golden):
    """At 2^20, check a handful of output positions against a direct
    DFT evaluation out[j] = sum_i a_i w^(ij) computed with Python bigints."""
    log_n = 20
    n = 1 << log_n
    r = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    R = 1 << 256

    def from_mont(b):
        return int.from_bytes(b, "little") * pow(R, -1, r) % r

    a = oracle.gen_fr_vector(n, 5555)
    w = _omega(log_n, oracle, golden)
    out = gpu.ntt(a, log_n, w)
    wv = from_mont(w)
    av = [from_mont(a[32 * i:32 * i + 32]) for i in range(n)]
    import random
    rng = random.Random(1)
    for j in [0, 1, n - 1] + [rng.randrange(n) for _ in range(2)]:
        wj = pow(wv, j, r)
        acc, cur = 0, 1
        for i in range(n):
            acc = (acc + av[i] * cur) % r
            cur = cur * wj % r
        got = from_mont(out[32 * j:32 * j + 32])
        assert got == acc, f"output {j}"


# ---------------------------------------------------------------- robustness
def test_concurrent_calls_one_ctx(gpu, oracle):
    """halo2 commits from concurrent rayon workers; the ctx must serialize
    safely and return correct results from every thread."""
    import threading
    n = 1024
    cases = []
    for seed in range(6):
        sc, bs = oracle.gen_msm_inputs(n, 800 + seed, fast=True)
        cases.append((sc, bs, oracle.msm(bs, sc, n)))
    errors = []

    def worker(sc, bs, want):
        try:
            for _ in range(3):
                got = gpu.msm(bs, sc, n)
                assert got == want
        except Exception as e:  # pragma: no cover
            errors.append(e)

    threads = [threading.Thread(target=worker, args=c) for c in cases]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors


def test_error_paths(gpu):
    import pytest as _pytest
    with _pytest.raises(RuntimeError, match="log_n"):
        gpu.ntt(b"\x00" * 32, 29, b"\x01" + b"\x00" * 31)
    with _pytest.raises(RuntimeError, match="nbatch"):
        gpu.msm_batch(b"\x00" * 64, b"\x00" * (33 * 32), 33, 1)
    # the batch bound holds before anything is sized by nbatch: with n = 0,
    # and on the device-pointer entry (refused before a pointer is read)
    with pytest.raises(RuntimeError, match="rc=-3: .*nbatch 33"):
        gpu.msm_batch(None, b"", 33, 0)
    d_b, d_s = gpu.malloc(64), gpu.malloc(33 * 32)
    try:
        for nbatch in (0, 33):
            with pytest.raises(RuntimeError,
                               match=f"rc=-3: .*nbatch {nbatch}"):
                gpu.msm_batch_device(d_b, d_s, nbatch, 1)
    finally:
        gpu.free(d_b)
        gpu.free(d_s)
    assert gpu.msm_batch(None, b"", 32, 0) == [bytes(64)] * 32


def _ntt_legs_vs_oracle_in_child(env, log_ns):
    """In a fresh child process (the split rule is fixed when the context is
    created) under `env` on top of the caller's environment minus
    SPECTRE_NTT_FORCE3: forward, inverse, forward-coset and inverse-coset
    NTT of every log_n must match the oracle bit-exactly."""
    import os
    import subprocess
    import sys
    REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import sys, os
sys.path.insert(0, %r); sys.path.insert(0, %r)
import pywrap as oracle
from spectre_amd import SpectreGpu
import json
fix = json.load(open(os.path.join(%r, "tests", "golden", "ntt.json")))
w12 = bytes.fromhex([c for c in fix["seeded_cases"] if c["log_n"] == 12][0]["omega_mont"])
gpu = SpectreGpu([0])
g = oracle.fr_from_canonical((5).to_bytes(32, "little"))
gi = oracle.fr_inv(g)
for log_n in %r:
    w = w12
    if log_n <= 12:
        for _ in range(12 - log_n):
            w = oracle.fr_mul(w, w)
    else:
        r = 21888242871839275222246405745257275088548364400416034343698204186575808495617
        g7 = oracle.fr_from_canonical((7).to_bytes(32, "little"))
        w = oracle.fr_pow(g7, ((r - 1) >> 28).to_bytes(32, "little"))
        for _ in range(28 - log_n):
            w = oracle.fr_mul(w, w)
    a = oracle.gen_fr_vector(1 << log_n, 600 + log_n)
    assert gpu.ntt(a, log_n, w) == oracle.ntt(a, log_n, w), log_n
    wi = oracle.fr_inv(w)
    assert gpu.ntt(a, log_n, wi, inverse=True) == oracle.ntt(a, log_n, wi, inverse=True), log_n
    assert gpu.ntt(a, log_n, w, coset_gen=g) == oracle.ntt(a, log_n, w, coset_gen=g), log_n
    assert (gpu.ntt(a, log_n, wi, inverse=True, coset_gen=gi)
            == oracle.ntt(a, log_n, wi, inverse=True, coset_gen=gi)), log_n
print("ntt legs ok")
''' % (REPO, REPO + "/oracle", REPO, tuple(log_ns))
    child_env = {k: v for k, v in os.environ.items()
                 if k != "SPECTRE_NTT_FORCE3"}
    child_env.update(env)
    r = subprocess.run([sys.executable, "-c", code], env=child_env,
                       capture_output=True, text=True, timeout=300)
    assert "ntt legs ok" in r.stdout, r.stdout + r.stderr


# sizes of the forced three-pass test (test_ntt_split.py reads the list)
FORCE3_LOG_NS = (3, 4, 5, 7, 6, 10, 12, 14)


def test_ntt_three_pass_forced_vs_oracle(oracle, golden):
    """The 3-pass (log_n>24) path, forced at oracle-checkable sizes via
    SPECTRE_NTT_FORCE3, must match the oracle bit-exactly (fwd/inv/coset,
    and the inverse coset on the scattered store). log_n 3, 4, 5, 7 split
    (1,1,1), (2,1,1), (2,2,1), (3,2,2): one-entry twiddle tables and unequal
    axes."""
    _ntt_legs_vs_oracle_in_child({"SPECTRE_NTT_FORCE3": "1"},
                                 FORCE3_LOG_NS)


# a second forced item (test_ntt_split.py reads this list too)
FORCE3_LARGE_LOG_NS = (21, 22)


def test_ntt_three_pass_forced_large_vs_oracle(oracle, golden):
    """Forced three passes at log_n 21 and 22, splits (7,7,7) and (8,7,7):
    the (7,7,middle), (7,0,last) and (8,7,middle) passes that 2^26 and 2^27
    end with, against the oracle itself on all four legs."""
    _ntt_legs_vs_oracle_in_child({"SPECTRE_NTT_FORCE3": "1"},
                                 FORCE3_LARGE_LOG_NS)


def test_ntt_two_pass_short_first_axis_vs_oracle(oracle, golden):
    """The default rule's (1,12) and (2,12) splits at log_n 13 and 14: a
    one- and a two-entry twiddle table on the strided pass, all four legs."""
    _ntt_legs_vs_oracle_in_child({}, (13, 14))


def test_ntt_2pow25_roundtrip(gpu, oracle, golden):
    """Aggregation-scale extended domain (>2^24): 3-pass path round trip
    and parity vs the oracle on a slice via linear DFT check is too slow;
    round trip + oracle comparison at full size (OpenMP oracle, ~seconds)."""
    log_n = 25
    n = 1 << log_n
    r = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    g7 = oracle.fr_from_canonical((7).to_bytes(32, "little"))
    w = oracle.fr_pow(g7, ((r - 1) >> 28).to_bytes(32, "little"))
    for _ in range(28 - log_n):
        w = oracle.fr_mul(w, w)
    wi = oracle.fr_inv(w)
    # copies of one chunk, each rotated by another odd element count, as
    # test_ntt_shapes_gpu.vec() builds them: plainly repeated, the vector has
    # period 2^20 and its DFT is zero at 31 outputs of 32, where no wrong
    # factor shows
    chunk = oracle.gen_fr_vector(1 << 20, 2525)
    parts = []
    for j in range(n >> 20):
        cut = 32 * ((j * 40503) % (1 << 20))
        parts.append(chunk[cut:] + chunk[:cut])
    a = b"".join(parts)
    d = gpu.malloc(32 * n)
    gpu.upload(d, a)
    gpu.ntt_device(d, log_n, w)
    out_gpu_head = gpu.download(d, 32 * 4096)  # spot region
    want = oracle.ntt(a, log_n, w)
    assert out_gpu_head == want[:32 * 4096]
    assert gpu.download(d, 32 * n) == want
    gpu.ntt_device(d, log_n, wi, inverse=True)
    assert gpu.download(d, 32 * n) == a
    gpu.free(d)


def _gate_ref():
    """tests/gate_ref.py, the bigint restatement of the gate-expression
    evaluator (the checker for SURVEY §8f-3), loaded by path."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "gate_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                 "gate_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gate_eval_vs_reference(gpu, oracle):
    """Gate-expression evaluator (quotient phase): the
    halo2-base flex-gate shape q*(a + b*c - d) over rotations of one
    column, plus random programs, vs the bigint restatement."""
    import random
    R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    gate_ref = _gate_ref()
    assert gate_ref.R == R
    n = 1 << 10
    rng = random.Random(8015)

    def fr_vec(ints):
        return b"".join(
            oracle.fr_from_canonical(v.to_bytes(32, "little")) for v in ints)

    def to_ints(raw):
        return [int.from_bytes(
            oracle.fr_to_canonical(raw[32 * i:32 * (i + 1)]), "little")
            for i in range(len(raw) // 32)]

    ncols = 3
    cols_int = [[rng.randrange(R) for _ in range(n)] for _ in range(ncols)]
    d_cols = []
    for ci in cols_int:
        d = gpu.malloc(32 * n)
        gpu.upload(d, fr_vec(ci))
        d_cols.append(d)
    d_out = gpu.malloc(32 * n)

    G = gpu
    # flex gate: q * (a + b*c - d) with a,b,c,d = rotations 0..3 of col 1,
    # q = col 0 (rot_scale 4 as the extended domain would use)
    flex = [(G.GATE_COL, 0, 0),
            (G.GATE_COL, 1, 0), (G.GATE_COL, 1, 1), (G.GATE_COL, 1, 2),
            (G.GATE_MUL, 0, 0), (G.GATE_ADD, 0, 0),
            (G.GATE_COL, 1, 3), (G.GATE_SUB, 0, 0),
            (G.GATE_MUL, 0, 0)]
    G.gate_eval(d_cols, b"", flex, n, rot_scale=4, d_out=d_out)
    want = gate_ref.eval_program(cols_int, [], flex, n, 4)
    assert to_ints(bytes(G.download(d_out, 32 * n))) == want

    # accumulate form out = out*y + v, with constants and negation
    y = rng.randrange(R)
    consts = [rng.randrange(R) for _ in range(2)]
    prog2 = [(G.GATE_CONST, 0, 0), (G.GATE_COL, 2, -1), (G.GATE_MUL, 0, 0),
             (G.GATE_CONST, 1, 0), (G.GATE_NEG, 0, 0), (G.GATE_ADD, 0, 0)]
    G.gate_eval(d_cols, fr_vec(consts), prog2, n, rot_scale=1,
                y=fr_vec([y]), d_out=d_out)
    want2 = gate_ref.eval_program(cols_int, consts, prog2, n, 1, y, want)
    assert to_ints(bytes(G.download(d_out, 32 * n))) == want2

    # random well-formed programs of a set depth, the maximum included
    for trial, depth in enumerate((8, 8, 7, 6, 4, 2)):
        consts = [rng.randrange(R) for _ in range(3)]
        prog, maxd = gate_ref.compile_tree(gate_ref.random_tree(
            rng, ncols, 3, range(-3, 4), depth))
        assert maxd == depth
        G.gate_eval(d_cols, fr_vec(consts), prog, n, rot_scale=2, d_out=d_out)
        want = gate_ref.eval_program(cols_int, consts, prog, n, 2)
        assert to_ints(bytes(G.download(d_out, 32 * n))) == want, trial

    # validation: malformed programs are rejected loudly
    import pytest as _pytest
    for bad in ([(G.GATE_ADD, 0, 0)],                     # underflow
                [(G.GATE_COL, 99, 0)],                    # bad column
                [(G.GATE_COL, 0, 0), (G.GATE_COL, 0, 0)],  # 2 left on stack
                [(G.GATE_COL, 0, 0)] * 9):                # depth > max
        with _pytest.raises(RuntimeError):
            G.gate_eval(d_cols, b"", bad, n, d_out=d_out)

    for d in d_cols + [d_out]:
        gpu.free(d)


def test_quotient_pipeline_device_resident(gpu, oracle):
    """The whole quotient phase device-resident: per-column
    iFFT -> coset-FFT, gate expression over the coset values, inverse-coset
    iFFT of the result — one upload, one download, bit-exact against the
    oracle NTTs + a bigint evaluation of the same expression."""
    R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    log_n = 10
    n = 1 << log_n
    # omega from the module ROOT28 (verified vs fixtures in test_root_consistency)
    w = ROOT28
    for _ in range(28 - log_n):
        w = oracle.fr_mul(w, w)
    wi = oracle.fr_inv(w)
    g5 = oracle.fr_from_canonical((5).to_bytes(32, "little"))
    g5i = oracle.fr_inv(g5)

    cols = [oracle.gen_fr_vector(n, 7000 + i) for i in range(3)]
    d_cols = []
    for cvec in cols:
        d = gpu.malloc(32 * n)
        gpu.upload(d, cvec)
        d_cols.append(d)
    d_out = gpu.malloc(32 * n)

    # device: evaluations -> coeffs -> coset evals, per column
    for d in d_cols:
        gpu.ntt_device(d, log_n, wi, inverse=True)
        gpu.ntt_device(d, log_n, w, coset_gen=g5)
    G = gpu
    flex = [(G.GATE_COL, 0, 0),
            (G.GATE_COL, 1, 0), (G.GATE_COL, 1, 1), (G.GATE_COL, 2, 2),
            (G.GATE_MUL, 0, 0), (G.GATE_ADD, 0, 0),
            (G.GATE_COL, 2, 3), (G.GATE_SUB, 0, 0),
            (G.GATE_MUL, 0, 0)]
    G.gate_eval(d_cols, b"", flex, n, rot_scale=4, d_out=d_out)
    gpu.ntt_device(d_out, log_n, wi, inverse=True, coset_gen=g5i)
    got = bytes(gpu.download(d_out, 32 * n))

    # oracle: identical sequence
    ref_cosets = []
    for cvec in cols:
        coeff = oracle.ntt(cvec, log_n, wi, inverse=True)
        ref_cosets.append(oracle.ntt(coeff, log_n, w, coset_gen=g5))

    def to_ints(raw):
        return [int.from_bytes(
            oracle.fr_to_canonical(raw[32 * i:32 * (i + 1)]), "little")
            for i in range(n)]
    ci = [to_ints(c) for c in ref_cosets]
    ev = _gate_ref().eval_program(ci, [], flex, n, 4)
    ev_bytes = b"".join(
        oracle.fr_from_canonical(v.to_bytes(32, "little")) for v in ev)
    want = oracle.ntt(ev_bytes, log_n, wi, inverse=True, coset_gen=g5i)
    assert got == want
    for d in d_cols + [d_out]:
        gpu.free(d)


def test_fr_vec_ops_vs_oracle(gpu, oracle):
    """Pointwise Fr vector ops (quotient gate-eval glue) vs the oracle."""
    n = 4097
    a = oracle.gen_fr_vector(n, 91)
    b = oracle.gen_fr_vector(n, 92)
    cst = oracle.gen_fr_vector(1, 93)
    d_a = gpu.malloc(32 * n)
    d_b = gpu.malloc(32 * n)
    d_o = gpu.malloc(32 * n)
    gpu.upload(d_a, a)
    gpu.upload(d_b, b)
    cases = [
        (gpu.VEC_ADD, None, oracle.fr_add),
        (gpu.VEC_SUB, None, oracle.fr_sub),
        (gpu.VEC_MUL, None, oracle.fr_mul),
    ]
    for op, c, fn in cases:
        gpu.fr_vec_op(op, d_a, d_b, c, d_o, n)
        got = gpu.download(d_o, 32 * n)
        want = b"".join(fn(a[32 * i:32 * i + 32], b[32 * i:32 * i + 32])
                        for i in range(n))
        assert got == want, op
    gpu.fr_vec_op(gpu.VEC_SCALE, d_a, None, cst, d_o, n)
    got = gpu.download(d_o, 32 * n)
    want = b"".join(oracle.fr_mul(a[32 * i:32 * i + 32], cst)
                    for i in range(n))
    assert got == want
    gpu.fr_vec_op(gpu.VEC_ADD_SCALED, d_a, d_b, cst, d_o, n)
    got = gpu.download(d_o, 32 * n)
    want = b"".join(
        oracle.fr_add(a[32 * i:32 * i + 32],
                      oracle.fr_mul(b[32 * i:32 * i + 32], cst))
        for i in range(n))
    assert got == want
    # in-place aliasing (out == a)
    gpu.fr_vec_op(gpu.VEC_ADD, d_a, d_b, None, d_a, n)
    got = gpu.download(d_a, 32 * n)
    want = b"".join(oracle.fr_add(a[32 * i:32 * i + 32], b[32 * i:32 * i + 32])
                    for i in range(n))
    assert got == want
    for p in (d_a, d_b, d_o):
        gpu.free(p)


def test_msm_randomized_sizes(gpu, oracle):
    """Seeded sweep over awkward sizes (odd, prime-ish, off-by-one around
    thread/partition boundaries) x scalar encodings — edge insurance for the
    equal-work partitioning and boundary-fixup logic."""
    import random
    rng = random.Random(20260915)
    sizes = [1, 2, 63, 64, 65, 255, 1000003 % 4096, 4095, 4097,
             rng.randrange(1, 20000), rng.randrange(1, 20000)]
    for idx, n in enumerate(sizes):
        sc, bs = oracle.gen_msm_inputs(n, 7000 + idx, fast=True)
        want = oracle.msm(bs, sc, n)
        assert gpu.msm(bs, sc, n) == want, (n, "canonical")
        scm = b"".join(
            oracle.fr_from_canonical(sc[32 * i:32 * i + 32])
            for i in range(n))
        assert gpu.msm(bs, scm, n, canonical=False) == want, (n, "mont")


def test_msm_batch_randomized(gpu, oracle):
    import random
    rng = random.Random(99)
    for trial in range(3):
        n = rng.randrange(100, 5000)
        nb = rng.randrange(2, 7)
        _, bs = oracle.gen_msm_inputs(n, 7100 + trial, fast=True)
        scal, singles = b"", []
        for b in range(nb):
            sc, _ = oracle.gen_msm_inputs(n, 7200 + 10 * trial + b, fast=True)
            scal += sc
            singles.append(oracle.msm(bs, sc, n))
        assert gpu.msm_batch(bs, scal, nb, n) == singles, (n, nb)
