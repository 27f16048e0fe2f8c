"""ff_add / ff_sub / ff_cond_sub_mod and ff_sqr of ff.hpp at the operands where
their two forms could part: the carry-chain form with its correction selected
by a mask (fields with kChainAddSub: Fq) against the 64-bit form with the
correction behind a branch (Fr, FrCios), and the 36-product column squaring
(device, Fq and Fr) against ff_mul(a, a) (host, and FrCios everywhere).

Through the probe library of tests/test_field_probe.py, unchanged: every case
runs on the host build of the headers without a GPU, and its twin marked
`gpu` in the kernels. Everything is bit-exact against Python bigints on
Montgomery images (tests/edge_operands.py); operands from
tests/chain_operands.py.

The curve ops are not repeated here: test_field_probe.py::test_device_curve
and ::test_host_curve already run g1_madd / g1_dbl / g1_add of the rebuilt
library over curve_cases() and dbl_cases() against the bigint sums.
"""
import pytest

import chain_operands as co
import edge_operands as eo
from test_field_probe import check_field, run_field

WHERE = ["host", pytest.param("device", marks=pytest.mark.gpu)]
FIELD_NAMES = list(eo.FIELDS)


def check(where, op, field, ps):
    m = eo.FIELDS[field]
    return check_field(where, op, field, ps,
                       [eo.expect(op, m, a, b) for a, b in ps])


# -------------------------------------------------------------------- add/sub
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_add_sub_at_the_reduction_boundary(where, field):
    """a + b in {m-1, m, m+1} and a - b in {-1, 0, 1}."""
    ps = co.boundary_pairs(eo.FIELDS[field])
    for op in ("add", "sub"):
        check(where, op, field, ps)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_add_sub_ripple_through_every_limb(where, field):
    ps = co.ripple_pairs(eo.FIELDS[field])
    for op in ("add", "sub"):
        check(where, op, field, ps)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("field", FIELD_NAMES)
@pytest.mark.parametrize("op", ["add", "sub"])
def test_correction_alternates_lane_by_lane(where, field, op):
    """One wave and a lane in which every other element takes the
    correction: the mask has to select what the branch selected."""
    m = eo.FIELDS[field]
    for which in ("add", "sub"):
        check(where, op, field, co.alternating65(m, which))


# ------------------------------------------------------------------------ sqr
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_sqr_at_the_doubled_limb_edges(where, field):
    """sqr is the bigint square and, byte for byte, mul(a, a)."""
    ps = [(a, a) for a in co.sqr_operands(eo.FIELDS[field])]
    got = check(where, "sqr", field, ps)
    assert got == run_field(where, "mul", field, ps), \
        f"{where} {field}: sqr and mul(a, a) differ"


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("field", FIELD_NAMES)
def test_sqrchain_from_the_doubled_limb_edges(where, field):
    """32 squarings back to back from each of them."""
    check(where, "sqrchain", field,
          [(a, a) for a in co.sqr_operands(eo.FIELDS[field])])
