"""CPU checks that pin tests/permutation_ref.py itself: on a generated valid
permutation the chained grand product over all rows closes to exactly 1, a
broken copy constraint opens it, and the chunk loop composes."""
import importlib.util
import os
import random

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "permutation_ref", os.path.join(HERE, "permutation_ref.py"))
pr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pr)
R = pr.R

# (log_n, columns, columns per chunk)
SHAPES = [(4, 3, 2), (9, 5, 2), (10, 3, 3)]


def setup(log_n, m, seed):
    rng = random.Random(seed)
    n = 1 << log_n
    omega = pr.ref.fr_root_of_unity(log_n)
    values, sigmas = pr.valid_permutation(m, n, omega, pr.DELTA, rng)
    return n, omega, values, sigmas, rng.randrange(R), rng.randrange(R)


@pytest.mark.parametrize("log_n,m,chunk", SHAPES)
def test_valid_permutation_closes_to_one(log_n, m, chunk):
    n, omega, values, sigmas, beta, gamma = setup(log_n, m, 0x9e3 + log_n)
    # sigma is a permutation of the identity labels delta^j * omega^i
    ids = sorted(pow(pr.DELTA, j, R) * pow(omega, i, R) % R
                 for j in range(m) for i in range(n))
    assert sorted(s for col in sigmas for s in col) == ids
    assert len(set(ids)) == m * n
    delta0 = 1
    for c0 in range(0, m, chunk):
        _, den = pr.terms(values[c0:c0 + chunk], sigmas[c0:c0 + chunk], beta,
                          gamma, omega, delta0, pr.DELTA, n)
        assert all(den), "a denominator is zero"
        delta0 = delta0 * pow(pr.DELTA, chunk, R) % R
    chunks = pr.commit_chunks(values, sigmas, chunk, beta, gamma, omega,
                              pr.DELTA, n, blinding=-1)
    assert len(chunks) == -(-m // chunk)
    assert all(len(z) == n for z, _ in chunks)
    assert chunks[0][0][0] == 1
    assert chunks[-1][1] == 1, "the chained product does not close"
    if len(chunks) > 1:
        assert chunks[0][1] != 1, "the first chunk alone should not close"


@pytest.mark.parametrize("log_n,m,chunk", SHAPES)
def test_broken_copy_constraint_opens_the_product(log_n, m, chunk):
    n, omega, values, sigmas, beta, gamma = setup(log_n, m, 0x9e3 + log_n)
    # a cell on a cycle of length >= 2: its sigma names another cell
    j, i = next((j, i) for j in range(m) for i in range(n)
                if sigmas[j][i] != pow(pr.DELTA, j, R) * pow(omega, i, R) % R)
    broken = [list(col) for col in values]
    broken[j][i] = (broken[j][i] + 1) % R
    chunks = pr.commit_chunks(broken, sigmas, chunk, beta, gamma, omega,
                              pr.DELTA, n, blinding=-1)
    assert chunks[-1][1] != 1


@pytest.mark.parametrize("blinding", [-1, 5])
def test_one_chunk_equals_two_chained_chunks_multiplied(blinding):
    log_n, m = 6, 4
    n, omega, values, sigmas, beta, gamma = setup(log_n, m, 77)
    (z_one, last_one), = pr.commit_chunks(values, sigmas, m, beta, gamma,
                                          omega, pr.DELTA, n, blinding)
    (za, la), (zb, lb) = pr.commit_chunks(values, sigmas, 2, beta, gamma,
                                          omega, pr.DELTA, n, blinding)
    u = n - blinding - 1
    assert len(z_one) == len(za) == len(zb) == u
    # the second chunk starts at the first's last_z: divide it out
    la_inv = pow(la, -1, R)
    assert zb[0] == la
    assert [a * b % R * la_inv % R for a, b in zip(za, zb)] == z_one
    assert lb == last_one


def test_chunk_loop_agrees_with_the_two_formulas():
    """commit_chunks' modified_values against terms(), chunk by chunk: the
    deltaomega carry is delta0 = delta^(first column of the chunk)."""
    log_n, m, chunk = 5, 5, 2
    n, omega, values, sigmas, beta, gamma = setup(log_n, m, 1234)
    blinding = 3
    u = n - blinding - 1
    chunks = pr.commit_chunks(values, sigmas, chunk, beta, gamma, omega,
                              pr.DELTA, n, blinding)
    last = 1
    for k, (z, last_z) in enumerate(chunks):
        c0 = k * chunk
        num, den = pr.terms(values[c0:c0 + chunk], sigmas[c0:c0 + chunk],
                            beta, gamma, omega, pow(pr.DELTA, c0, R),
                            pr.DELTA, n)
        acc, want = last, []
        for i in range(u):
            want.append(acc)
            acc = acc * num[i] % R * pr.inv0(den[i]) % R
        assert z == want and last_z == acc
        last = last_z


def test_powers_and_encoding():
    g, c = 0x1234567, R - 5
    assert pr.powers(c, g, 4) == [c, c * g % R, c * g * g % R,
                                  c * pow(g, 3, R) % R]
    assert pr.powers(c, 0, 3) == [c, 0, 0]
    assert pr.powers(1, g, 0) == []
    vals = [0, 1, R - 1, g]
    assert pr.ints(pr.mont(vals)) == vals
