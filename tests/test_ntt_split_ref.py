"""tests/ntt_split_ref.py WITHOUT a GPU: the split identity in Python
integers against an O(n^2) DFT, the whole reference through the host backend
against oracle.ntt on the full vector, and that a wrong coefficient table
fails the comparison."""
import random

import pytest

import ntt_split_ref as sr
import test_ntt_shapes_gpu as shapes

R = sr.R


def wrong_zeta_exponent(form: sr.Form, enc=lambda v: v) -> sr.Form:
    """The form with zeta^(i1*(j1+1)) where zeta^(i1*j1) belongs."""
    zeta = pow(form_w(form), (1 << form.log_n) // form.n1, R)
    return form._replace(coeffs=[
        [enc(c * pow(zeta, i1, R) % R) for i1, c in enumerate(row)]
        for row in form.coeffs])


def form_w(form: sr.Form) -> int:
    """w of an integer form: gens[1] / gens[0]."""
    return form.gens[1] * pow(form.gens[0], -1, R) % R


def test_leg_ints_are_leg_args():
    """The legs' omega and generator are the ones test_ntt_shapes_gpu runs."""
    for log_n in (5, 12, 25, 28):
        for leg in sr.DIRECT_LEGS:
            w, g, scale = sr.leg_ints(log_n, leg)
            omega, inverse, gen = shapes.leg_args(log_n, leg)
            assert sr.enc(w) == omega
            assert (gen is None and g == 1) or sr.enc(g) == gen
            assert scale == (pow(1 << log_n, -1, R) if inverse else 1)


@pytest.mark.parametrize("leg", sr.DIRECT_LEGS)
@pytest.mark.parametrize("log_n,n1", [(5, 2), (6, 4), (7, 8)])
def test_identity_in_integers_vs_quadratic_dft(log_n, n1, leg):
    rng = random.Random(9100 + log_n)
    x = [rng.randrange(R) for _ in range(1 << log_n)]
    x[0], x[-1] = 0, R - 1
    w, g, scale = sr.leg_ints(log_n, leg)
    X = sr.dft_ints(x, w, g, scale)
    form = sr.leg_form(log_n, n1, leg)
    assert sr.mismatches(sr.IntBackend(), x, X, form) == []
    # every slice of a wrong table differs, and so does one wrong output
    bad = wrong_zeta_exponent(form)
    assert sr.mismatches(sr.IntBackend(), x, X, bad) == list(range(n1))
    X[n1 + 1] = (X[n1 + 1] + 1) % R
    assert sr.mismatches(sr.IntBackend(), x, X, form) == [1]


def test_inverse_leg_undoes_the_forward_leg_in_integers():
    rng = random.Random(9200)
    x = [rng.randrange(R) for _ in range(32)]
    assert sr.dft_ints(sr.dft_ints(x, *sr.leg_ints(5, "fwd")),
                       *sr.leg_ints(5, "inv")) == x


_full = {}


def full(oracle, log_n, leg):
    """(x, oracle.ntt(x)) of a leg at 2^log_n, computed once."""
    if (log_n, leg) not in _full:
        x = oracle.gen_fr_vector(1 << log_n, seed=9300 + log_n)
        omega, inverse, gen = shapes.leg_args(log_n, leg)
        _full[log_n, leg] = (x, oracle.ntt(x, log_n, omega, inverse=inverse,
                                           coset_gen=gen))
    return _full[log_n, leg]


@pytest.mark.parametrize("leg", sr.DIRECT_LEGS)
@pytest.mark.parametrize("log_n,n1", [(12, 4), (12, 32), (14, 8)])
def test_host_backend_vs_oracle_on_the_full_vector(oracle, log_n, n1, leg):
    x, X = full(oracle, log_n, leg)
    form = sr.leg_form_mont(log_n, n1, leg)
    assert sr.mismatches(sr.HostBackend(oracle), x, X, form) == []


@pytest.mark.parametrize("leg", sr.DIRECT_LEGS)
def test_wrong_coefficient_table_fails_the_host_comparison(oracle, leg):
    log_n, n1 = 12, 4
    x, X = full(oracle, log_n, leg)
    bad = sr.mont_form(wrong_zeta_exponent(sr.leg_form(log_n, n1, leg)))
    assert sr.mismatches(sr.HostBackend(oracle), x, X, bad) == list(range(n1))


def test_one_wrong_element_fails_its_slice_only(oracle):
    log_n, n1 = 12, 32
    x, X = full(oracle, log_n, "coset")
    k = n1 * 77 + 13
    X = X[:32 * k] + sr.enc(1) + X[32 * k + 32:]
    form = sr.leg_form_mont(log_n, n1, "coset")
    assert sr.mismatches(sr.HostBackend(oracle), x, X, form) == [13]
