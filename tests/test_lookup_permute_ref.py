"""The two forms of the lookup permutation in tests/lookup_permute_ref.py
agree, and a successful result has the properties the lookup argument needs.
CPU only: this is the check of the reference the GPU tests compare against,
and of the identity between halo2's serial walk and the parallel form that
lookup.hip runs."""
import random

import lookup_permute_ref as lp

R = lp.R


def random_case(rng):
    """A small multiset pair. Few distinct values, so that repeats, exhausted
    table values and misses are all common; values from the whole field now
    and then so that the order is not the order of small integers alone."""
    u = rng.randrange(0, 24)
    pool_n = rng.randrange(1, 9)
    if rng.random() < 0.3:
        pool = [rng.randrange(R) for _ in range(pool_n)]
    else:
        pool = rng.sample(range(12), pool_n)
    s = [rng.choice(pool) for _ in range(u)]
    kind = rng.random()
    if kind < 0.6 and u:       # inputs from the table: succeeds
        a = [rng.choice(s) for _ in range(u)]
    elif kind < 0.8:           # inputs from the pool: may miss
        a = [rng.choice(pool) for _ in range(u)]
    else:                      # anything nearby: usually misses
        a = [rng.randrange(14) for _ in range(u)]
    return a, s


def run(form, a, s):
    try:
        return form(a, s)
    except lp.LookupMiss as e:
        return ("miss", e.missing)


def test_serial_and_parallel_forms_agree():
    rng = random.Random(20240)
    ok = missed = 0
    for _ in range(4000):
        a, s = random_case(rng)
        got_serial = run(lp.serial, a, s)
        assert run(lp.parallel, a, s) == got_serial, (a, s)
        if got_serial[0] == "miss":
            missed += 1
            assert got_serial[1] == len(set(a) - set(s))
            continue
        ok += 1
        a_perm, s_perm = got_serial
        lp.check_properties(a, s, a_perm, s_perm, rng.randrange(R),
                            rng.randrange(R))
    # the generator reaches both outcomes often enough to mean something
    assert ok > 1500 and missed > 500, (ok, missed)


def test_hand_worked_example():
    """A = [3 1 3 3 2 1], S = [1 2 3 5 5 9]: A' = [1 1 2 3 3 3]; rows 0, 2, 3
    are first occurrences; 5, 5, 9 are left and go to the repeated rows 5, 4,
    1 in that order (smallest value to the last repeated row)."""
    a, s = [3, 1, 3, 3, 2, 1], [1, 2, 3, 5, 5, 9]
    want = ([1, 1, 2, 3, 3, 3], [1, 9, 2, 3, 5, 5])
    assert lp.serial(a, s) == want
    assert lp.parallel(a, s) == want


def test_empty_and_single():
    assert lp.serial([], []) == ([], []) == lp.parallel([], [])
    assert lp.serial([7], [7]) == ([7], [7]) == lp.parallel([7], [7])
    for form in (lp.serial, lp.parallel):
        assert run(form, [7], [8]) == ("miss", 1)
        assert run(form, [1, 5, 5, 9], [2, 2, 5, 5]) == ("miss", 2)


def test_codec_round_trip():
    vals = [0, 1, R - 1, 1 << 64, (1 << 192) + 5]
    assert lp.ints(lp.mont(vals)) == vals
    assert len(lp.enc(3)) == 32
