"""Reference for spectre_gpu_fr_powers / spectre_gpu_fr_permutation_terms on
plain Python integers: the permutation argument of the published PSE halo2
(plonk/permutation/prover.rs, keygen.rs and evaluation.rs), restated.

  powers()         c * g^i
  terms()          the two per-row products of one chunk of columns,
                     den[i] = prod_j (v_j[i] + beta*sigma_j[i]        + gamma)
                     num[i] = prod_j (v_j[i] + beta*delta0*delta^j*omega^i + gamma)
  commit_chunks()  halo2's chunk loop: modified_values (the denominators,
                   batch-inverted with zero staying zero, times the numerators
                   built with the deltaomega carry), the running product that
                   starts at last_z, and last_z = z[u] with u = n - blinding - 1
  valid_permutation()  columns and sigma columns that satisfy a random set of
                   copy constraints, as keygen's Assembly builds them

Values are canonical integers; ints() / mont() decode and encode the 32-byte
Montgomery images the library moves, with tests/golden/bn254_ref.py loaded by
path. Users must leave what these functions return unchanged."""
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "bn254_ref", os.path.join(HERE, "golden", "bn254_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
R = ref.R
MONT_INV = pow(ref.MONT, -1, R)
# halo2curves' Fr::DELTA = GENERATOR^(2^S): its order is the odd part of r - 1,
# so the cosets delta^j * <omega> of the columns are disjoint.
DELTA = pow(ref.FR_GEN, 1 << ref.FR_TWO_ADICITY, R)
assert DELTA == int(
    "09226b6e22c6f0ca64ec26aad4c86e715b5f898e5e963f25870e56bbe533e9a2", 16)
assert pow(DELTA, (R - 1) >> ref.FR_TWO_ADICITY, R) == 1


def ints(data: bytes) -> list[int]:
    return [int.from_bytes(data[i:i + 32], "little") * MONT_INV % R
            for i in range(0, len(data), 32)]


def enc(v: int) -> bytes:
    return ref.to_mont_bytes(v % R, R)


def mont(vals) -> bytes:
    return b"".join(enc(v) for v in vals)


def inv0(x: int) -> int:
    """ff::BatchInvert on one element: zero stays zero."""
    return pow(x, -1, R) if x else 0


def powers(c: int, g: int, n: int) -> list[int]:
    out, acc = [], c % R
    for _ in range(n):
        out.append(acc)
        acc = acc * g % R
    return out


def terms(values, sigmas, beta, gamma, omega, delta0, delta, n):
    """(num, den) over rows 0..n of one chunk: values / sigmas are lists of m
    columns, delta0 = delta^(index of the chunk's first column)."""
    assert len(values) == len(sigmas) >= 1
    num, den = [1] * n, [1] * n
    w = powers(1, omega, n)
    bd = beta * delta0 % R
    for v, s in zip(values, sigmas):
        for i in range(n):
            den[i] = den[i] * ((v[i] + beta * s[i] + gamma) % R) % R
            num[i] = num[i] * ((v[i] + bd * w[i] + gamma) % R) % R
        bd = bd * delta % R
    return num, den


def commit_chunks(values, sigmas, chunk, beta, gamma, omega, delta, n,
                  blinding):
    """halo2's permutation::prover::commit over all columns, `chunk` columns
    per Z column (cs_degree - 2). Returns [(z[0..u], last_z)] per chunk, u =
    n - blinding - 1; rows u.. of a Z column are last_z and the blinding rows,
    which the caller writes. blinding = -1 runs the product over all n rows
    (u = n), where a valid permutation closes it to 1."""
    u = n - blinding - 1
    assert 0 <= u <= n
    out = []
    deltaomega = 1  # delta^(columns done); the omega^row part is per row
    last_z = 1
    for c0 in range(0, len(values), chunk):
        cols = range(c0, min(c0 + chunk, len(values)))
        modified_values = [1] * n
        for j in cols:
            v, s = values[j], sigmas[j]
            for i in range(n):
                modified_values[i] = modified_values[i] * (
                    (beta * s[i] + gamma + v[i]) % R) % R
        modified_values = [inv0(x) for x in modified_values]
        for j in cols:
            v = values[j]
            row = deltaomega
            for i in range(n):
                modified_values[i] = modified_values[i] * (
                    (row * beta + gamma + v[i]) % R) % R
                row = row * omega % R
            deltaomega = deltaomega * delta % R
        z = [last_z]
        for row in range(1, u + 1):
            z.append(z[row - 1] * modified_values[row - 1] % R)
        last_z = z[u]
        out.append((z[:u], last_z))
    return out


def valid_permutation(m, n, omega, delta, rng):
    """(values, sigmas): the m * n cells are cut into random cycles of length
    1..7, every cell of a cycle holds the same random value, and sigma_j[i] =
    delta^j' * omega^i' names the successor (j', i') of cell (j, i) on its
    cycle: keygen's permutation polynomials for those copy constraints."""
    cells = [(j, i) for j in range(m) for i in range(n)]
    rng.shuffle(cells)
    w = powers(1, omega, n)
    d = powers(1, delta, m)
    values = [[None] * n for _ in range(m)]
    sigmas = [[None] * n for _ in range(m)]
    pos = 0
    while pos < len(cells):
        cyc = cells[pos:pos + rng.randint(1, 7)]
        pos += len(cyc)
        val = rng.randrange(R)
        for k, (j, i) in enumerate(cyc):
            nj, ni = cyc[(k + 1) % len(cyc)]
            values[j][i] = val
            sigmas[j][i] = d[nj] * w[ni] % R
    return values, sigmas
