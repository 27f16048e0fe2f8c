"""The host fold of the MSM reduction tail, without a GPU.

The device leaves three Jacobian partials per window; the library folds them
into the window sum  p0 + CHUNK * (p1 + LO * p2).  Here the fold gets points
with Z = 1 (and the identity in every combination of places) and its result,
made affine by the window combine, must equal the oracle's MSM over the same
points with the scalars (1, CHUNK, CHUNK * LO)."""
import itertools

import pytest

IDENT_JAC = bytes(96)  # Z = 0
IDENT_AFF = bytes(64)


def _fq_one(oracle):
    x = bytes([2] + [0] * 31)
    return oracle.fq_mul(x, oracle.fq_inv(x))  # Montgomery 1


def _affine_of(window_sum: bytes) -> bytes:
    """The fold's result as window 0 of an otherwise empty MSM."""
    from spectre_amd import ffi
    blob = window_sum + IDENT_JAC * (ffi.NUM_WINDOWS - 1)
    return ffi.combine_window_partials(blob, 1)


@pytest.fixture(scope="module")
def points(golden):
    pts = []
    for c in golden("g1.json")["mul_cases"]:
        p = bytes.fromhex(c["mul"])
        if p != IDENT_AFF and p not in pts:
            pts.append(p)
    assert len(pts) >= 4
    return pts


def _want(oracle, affine3):
    from spectre_amd import ffi
    weights = (1, ffi.MSM_TAIL_CHUNK, ffi.MSM_TAIL_CHUNK * ffi.MSM_TAIL_LO)
    want = IDENT_AFF
    for p, k in zip(affine3, weights):
        if p != IDENT_AFF:
            want = oracle.g1_add(want, oracle.g1_mul(p, k.to_bytes(32, "little")))
    # the same through the oracle's MSM over the points that are present
    live = [(p, k) for p, k in zip(affine3, weights) if p != IDENT_AFF]
    if live:
        bases = b"".join(p for p, _ in live)
        scalars = b"".join(k.to_bytes(32, "little") for _, k in live)
        assert oracle.msm(bases, scalars, len(live)) == want
    return want


def test_tail_constants_match_window_layout():
    from spectre_amd import ffi
    per_window = 1 << (ffi.WINDOW_BITS - 1)
    assert ffi.MSM_TAIL_CHUNK * ffi.MSM_TAIL_LO * ffi.MSM_TAIL_HI == per_window


def test_fold_window_symbol_declared():
    import os
    from spectre_amd import ffi
    assert hasattr(ffi.load_library(), "spectre_gpu_msm_fold_window")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "spectre_gpu.h")) as f:
        assert "spectre_gpu_msm_fold_window(" in f.read()


def test_fold_window_matches_oracle(oracle, points):
    from spectre_amd import ffi
    one = _fq_one(oracle)
    for trio in (points[0:3], points[1:4], [points[0]] * 3,
                 [points[2], oracle.g1_neg(points[2]), points[3]]):
        got = ffi.msm_fold_window(*(p + one for p in trio))
        assert _affine_of(got) == _want(oracle, trio)


def test_fold_window_with_identity_inputs(oracle, points):
    """One, two or all three partials are the identity."""
    from spectre_amd import ffi
    one = _fq_one(oracle)
    for mask in itertools.product((False, True), repeat=3):
        if not any(mask):
            continue
        trio = [IDENT_AFF if m else p for m, p in zip(mask, points)]
        jac = [IDENT_JAC if p == IDENT_AFF else p + one for p in trio]
        got = ffi.msm_fold_window(*jac)
        assert _affine_of(got) == _want(oracle, trio), mask
    assert _affine_of(ffi.msm_fold_window(IDENT_JAC, IDENT_JAC, IDENT_JAC)) \
        == IDENT_AFF


def test_fold_window_cancels_to_identity(oracle, points):
    """p0 = -(CHUNK * p1): the last add meets its own negative."""
    from spectre_amd import ffi
    one = _fq_one(oracle)
    k = ffi.MSM_TAIL_CHUNK.to_bytes(32, "little")
    p0 = oracle.g1_neg(oracle.g1_mul(points[0], k))
    got = ffi.msm_fold_window(p0 + one, points[0] + one, IDENT_JAC)
    assert _affine_of(got) == IDENT_AFF
