"""The NTT split rule (spectre_gpu_ntt_split, host-only) WITHOUT a GPU: its
invariants, the measured table it encodes, and that the GPU parity tests
reach every class of pass the rule produces.

What k_ntt_pass does in a pass follows from (logL, logS, position): the tile
size, the stride 2^logS (the sum of the later axes) and whether the pass is
the only, first, a middle or the last one. Radix-4 (logL >= 9, the tile at
which every thread of the launch has a quad) and the lone radix-2 level (odd
logL) follow from logL."""
import os

import pytest

import test_gpu_parity
import test_ntt_extend_gpu
import test_ntt_shapes_gpu
import test_ntt_three_axis_gpu
from spectre_amd import ffi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the default rule as ntt.hip's comments state the measured choices:
# one pass up to 2^12; k[1] = 12 up to 2^20, balanced above; three balanced
# axes at 2^25; k[0] = 12 from 2^26, the rest balanced
TABLE = {log_n: (log_n,) for log_n in range(1, 13)}
TABLE.update({log_n: (log_n - 12, 12) for log_n in range(13, 21)})
TABLE.update({21: (10, 11), 22: (11, 11), 23: (11, 12), 24: (12, 12),
              25: (9, 8, 8), 26: (12, 7, 7), 27: (12, 8, 7), 28: (12, 8, 8)})
THREE_AXIS = range(25, 29)
# the sizes the forced three-pass tests run, and the splits their docstrings
# name
FORCE3_SIZES = (3, 4, 5, 6, 7, 10, 12, 14, 21, 22)
FORCE3_TABLE = {3: (1, 1, 1), 4: (2, 1, 1), 5: (2, 2, 1), 7: (3, 2, 2),
                21: (7, 7, 7), 22: (8, 7, 7)}


def classes(split):
    """[(logL, logS, position)] of a split, in pass order."""
    out = []
    for i, k in enumerate(split):
        if len(split) == 1:
            pos = "only"
        else:
            pos = ("first" if i == 0 else
                   "last" if i == len(split) - 1 else "middle")
        out.append((k, sum(split[i + 1:]), pos))
    return out


def uncovered(required, reached):
    """[(log_n, class)] of the required {log_n: split} whose class no split
    in `reached` has."""
    have = {c for s in reached for c in s}
    return [(log_n, c) for log_n, split in sorted(required.items())
            for c in classes(split) if c not in have]


def test_symbol_exported_and_declared():
    assert hasattr(ffi.load_library(), "spectre_gpu_ntt_split")
    with open(os.path.join(REPO, "include", "spectre_gpu.h")) as f:
        assert "spectre_gpu_ntt_split(" in f.read()


@pytest.mark.parametrize("force3", [False, True])
def test_invariants(force3):
    for log_n in range(1, 29):
        k = ffi.ntt_split(log_n, force3)
        where = (log_n, force3, k)
        assert sum(k) == log_n, where
        assert all(1 <= x <= 12 for x in k), where
        if force3 and log_n >= 3:
            assert len(k) == 3, where
        else:
            assert len(k) == (1 if log_n <= 12 else 2 if log_n <= 24 else 3), where


def test_out_of_range_is_zero_passes():
    for force3 in (False, True):
        assert ffi.ntt_split(0, force3) == ()
        assert ffi.ntt_split(29, force3) == ()
        assert ffi.ntt_split(0xffffffff, force3) == ()


def test_default_table():
    for log_n, split in TABLE.items():
        assert ffi.ntt_split(log_n) == split, log_n
    assert set(TABLE) == set(range(1, 29))


def test_forced_table():
    for log_n, split in FORCE3_TABLE.items():
        assert ffi.ntt_split(log_n, force3=True) == split, log_n


def test_classes_of_a_split():
    assert classes((11,)) == [(11, 0, "only")]
    assert classes((3, 12)) == [(3, 12, "first"), (12, 0, "last")]
    assert classes((9, 8, 8)) == [(9, 16, "first"), (8, 8, "middle"),
                                  (8, 0, "last")]


def test_shape_list_covers_the_default_rule():
    """Every class of pass at log_n 1..24 is one that a size of
    test_ntt_shapes_gpu.SHAPES runs."""
    required = {log_n: ffi.ntt_split(log_n) for log_n in range(1, 25)}
    reached = [classes(ffi.ntt_split(s)) for s in test_ntt_shapes_gpu.SHAPES]
    missing = uncovered(required, reached)
    assert not missing, f"(log_n, class) no shape reaches: {missing}"
    # and the reverse: no shape outside the rule's range
    assert {c for s in reached for c in s} == {
        c for split in required.values() for c in classes(split)}


def test_coverage_check_sees_a_missing_shape():
    """The check above fails for each single log_n taken out of SHAPES."""
    required = {log_n: ffi.ntt_split(log_n) for log_n in range(1, 25)}
    for gone in range(1, 25):
        reached = [classes(ffi.ntt_split(s))
                   for s in test_ntt_shapes_gpu.SHAPES if s != gone]
        assert gone in {log_n for log_n, _ in uncovered(required, reached)}, gone


def three_axis_reached(sizes):
    """The classes test_ntt_three_axis_gpu runs with `sizes` as its size
    list. The extend cases' first pass is the EXT instantiation, other code,
    so only their later passes count."""
    reached = [classes(ffi.ntt_split(s)) for s in sizes]
    reached += [classes(ffi.ntt_split(log_n + ext))[1:]
                for log_n, ext in test_ntt_three_axis_gpu.EXTEND]
    return reached


def test_three_axis_list_covers_25_to_28():
    """Every class of pass at log_n 25..28 is one that a size of
    test_ntt_three_axis_gpu.SIZES runs, its extend cases reach the same
    sizes, and the sub-transform its reference rests on is a size that
    test_ntt_shapes_gpu compares with the oracle."""
    required = {log_n: ffi.ntt_split(log_n) for log_n in THREE_AXIS}
    assert all(len(split) == 3 for split in required.values())
    reached = three_axis_reached(test_ntt_three_axis_gpu.SIZES)
    missing = uncovered(required, reached)
    assert not missing, f"(log_n, class) no size reaches: {missing}"
    assert {c for s in reached for c in s} == {
        c for split in required.values() for c in classes(split)}
    assert {log_n + ext for log_n, ext in test_ntt_three_axis_gpu.EXTEND} == set(
        THREE_AXIS)
    assert test_ntt_three_axis_gpu.SUB_LOG in test_ntt_shapes_gpu.LARGE
    assert (test_ntt_three_axis_gpu.MACHINERY_LOG - 2
            in test_ntt_shapes_gpu.FULL)


def test_three_axis_check_sees_a_missing_size():
    """The check above fails for each single log_n taken out of SIZES: the
    first pass of every size is a class of its own."""
    required = {log_n: ffi.ntt_split(log_n) for log_n in THREE_AXIS}
    for gone in THREE_AXIS:
        reached = three_axis_reached(
            s for s in test_ntt_three_axis_gpu.SIZES if s != gone)
        assert gone in {log_n for log_n, _ in uncovered(required, reached)}, gone


def test_forced_lists_cover_the_forced_rule():
    """Every class of pass the three-axis rule has at FORCE3_SIZES is one the
    forced tests run. The extend test's first pass is the EXT instantiation,
    other code, so only its later passes count."""
    required = {log_n: ffi.ntt_split(log_n, force3=True)
                for log_n in FORCE3_SIZES}
    reached = [classes(ffi.ntt_split(s, force3=True))
               for s in (test_gpu_parity.FORCE3_LOG_NS
                         + test_gpu_parity.FORCE3_LARGE_LOG_NS)]
    reached += [classes(ffi.ntt_split(log_n + ext, force3=True))[1:]
                for log_n, ext in test_ntt_extend_gpu.FORCE3]
    missing = uncovered(required, reached)
    assert not missing, f"(log_n, class) no forced test reaches: {missing}"
    assert {c for s in reached for c in s} == {
        c for split in required.values() for c in classes(split)}
