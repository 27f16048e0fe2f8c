"""A reference for NTTs too large for the oracle: the DFT at n = n1 * n2 split
into n1 sub-transforms at n2, each of which is a call the suite has already
compared with the oracle at its own size. Not a test module;
tests/test_ntt_split_ref.py pins it on the CPU and
tests/test_ntt_three_axis_gpu.py compares the three-axis NTT with it.

With w a primitive n-th root, zeta = w^n2, g the coset generator (1: none),
j1 < n1, j2 < n2 and the sum over i1 < n1:

    X[n1*j2 + j1] = DFT_n2(u_j1; root w^n1, coset generator g*w^j1)[j2]
    u_j1[i2]      = sum_i1 zeta^(i1*j1) * g^(n2*i1) * x[i2 + n2*i1]

(write i = i2 + n2*i1 and k = n1*j2 + j1 in sum_i g^i x[i] w^(i*k); the
factor w^(n2*i1*n1*j2) is one). u_j1 is one linear combination of the n1
contiguous blocks of x, the sub-transform one forward coset NTT at n2, and
the result is the stride-n1 slice of X that starts at j1.

The legs (omega and g = 5 as test_ntt_shapes_gpu.leg_args takes them):
    fwd     the identity with g = 1
    coset   the identity with g = 5
    inv     the identity with w -> w^-1 and every coefficient times n^-1; the
            sub-transform stays a forward call with root (w^-1)^n1 and coset
            generator w^-j1, so the n^-1 of the transform under test is
            compared with one computed here in Python integers
The inverse coset leg has no form of its own: icoset(coset(x)) == x is
checked by the caller.

The reference is written once, in mismatches(), over a backend with three
operations:
    lincomb(x, n1, coeffs)        -> u, the combination of x's n1 blocks
    ntt(u, log_n2, root, gen)     -> u transformed (forward, coset gen)
    equal(X, n1, j1, u)           -> whether X[j1::n1] == u
IntBackend works on lists of Python integers with an O(n^2) DFT, HostBackend
on Montgomery bytes with oracle.ntt, DeviceBackend on torch int64 tensors
(four limbs per element; torch is plumbing only) through SpectreGpu's
fr_lincomb and ntt_device on raw pointers."""
import importlib.util
import os
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "bn254_ref", os.path.join(HERE, "golden", "bn254_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
R = ref.R
MONT_INV = pow(ref.MONT, -1, R)

DIRECT_LEGS = ("fwd", "coset", "inv")
COSET_GEN = 5

# coeffs[j1][i1], root of the sub-transform, gens[j1]: its coset generators
Form = namedtuple("Form", "log_n n1 coeffs root gens")


def enc(v: int) -> bytes:
    return ref.to_mont_bytes(v % R, R)


def ints(data: bytes) -> list[int]:
    return [int.from_bytes(data[i:i + 32], "little") * MONT_INV % R
            for i in range(0, len(data), 32)]


def mont(vals) -> bytes:
    return b"".join(enc(v) for v in vals)


def leg_ints(log_n: int, leg: str):
    """(w, g, scale) of a direct leg in integers: X[k] = scale * sum_i g^i
    x[i] w^(i*k)."""
    assert leg in DIRECT_LEGS, leg
    w = ref.fr_root_of_unity(log_n)
    if leg == "inv":
        return pow(w, -1, R), 1, pow(1 << log_n, -1, R)
    return w, COSET_GEN if leg == "coset" else 1, 1


def leg_form(log_n: int, n1: int, leg: str) -> Form:
    """The split of a leg at 2^log_n into n1 sub-transforms, in integers."""
    n = 1 << log_n
    assert n1 >= 1 and n % n1 == 0
    n2 = n // n1
    w, g, scale = leg_ints(log_n, leg)
    zeta, gn2 = pow(w, n2, R), pow(g, n2, R)
    coeffs = [[pow(zeta, i1 * j1, R) * pow(gn2, i1, R) * scale % R
               for i1 in range(n1)] for j1 in range(n1)]
    gens = [g * pow(w, j1, R) % R for j1 in range(n1)]
    return Form(log_n, n1, coeffs, pow(w, n1, R), gens)


def mont_form(form: Form) -> Form:
    """The same form with every field element as Montgomery bytes."""
    return form._replace(coeffs=[[enc(c) for c in row] for row in form.coeffs],
                         root=enc(form.root),
                         gens=[enc(g) for g in form.gens])


def leg_form_mont(log_n: int, n1: int, leg: str) -> Form:
    return mont_form(leg_form(log_n, n1, leg))


def mismatches(be, x, X, form: Form) -> list[int]:
    """The j1 whose slice X[j1::n1] is not what the split gives for x: empty
    when X is the transform of x. The field elements of `form` are in the
    backend's representation."""
    log_n2 = form.log_n - (form.n1.bit_length() - 1)
    assert form.n1 << log_n2 == 1 << form.log_n
    bad = []
    for j1 in range(form.n1):
        u = be.lincomb(x, form.n1, form.coeffs[j1])
        u = be.ntt(u, log_n2, form.root, form.gens[j1])
        if not be.equal(X, form.n1, j1, u):
            bad.append(j1)
        del u
    return bad


def dft_ints(x, w: int, g: int = 1, scale: int = 1) -> list[int]:
    """O(n^2): X[k] = scale * sum_i g^i x[i] w^(i*k)."""
    n = len(x)
    gx = [pow(g, i, R) * v % R for i, v in enumerate(x)]
    wp = [pow(w, e, R) for e in range(n)]
    return [scale * sum(v * wp[i * k % n] for i, v in enumerate(gx)) % R
            for k in range(n)]


class IntBackend:
    """Lists of integers; the form of leg_form()."""

    def lincomb(self, x, n1, coeffs):
        n2 = len(x) // n1
        return [sum(c * x[i2 + n2 * i1] for i1, c in enumerate(coeffs)) % R
                for i2 in range(n2)]

    def ntt(self, u, log_n2, root, gen):
        assert len(u) == 1 << log_n2 and pow(root, len(u), R) == 1
        return dft_ints(u, root, gen)

    def equal(self, X, n1, j1, u):
        return X[j1::n1] == u


class HostBackend:
    """Montgomery bytes; the lincomb in integers, the sub-transform by the
    oracle. The form of leg_form_mont()."""

    def __init__(self, oracle):
        self.oracle = oracle

    def lincomb(self, x, n1, coeffs):
        return mont(IntBackend().lincomb(ints(x), n1, ints(b"".join(coeffs))))

    def ntt(self, u, log_n2, root, gen):
        return self.oracle.ntt(u, log_n2, root, coset_gen=gen)

    def equal(self, X, n1, j1, u):
        step = 32 * n1
        return b"".join(X[o:o + 32]
                        for o in range(32 * j1, len(X), step)) == u


class DeviceBackend:
    """torch.int64 tensors of 4 * n limbs on the device, handed to the
    library as raw pointers. The library works on a stream of its own and
    synchronizes before it returns, so torch's work is synchronized before
    every call. The form of leg_form_mont()."""

    def __init__(self, gpu, torch):
        self.gpu, self.torch = gpu, torch

    def lincomb(self, x, n1, coeffs):
        n2 = x.numel() // 4 // n1
        u = self.torch.empty(4 * n2, dtype=self.torch.int64, device=x.device)
        ptrs = [x.data_ptr() + 32 * n2 * i1 for i1 in range(n1)]
        self.torch.cuda.synchronize()
        self.gpu.fr_lincomb(ptrs, coeffs, u.data_ptr(), n2)
        return u

    def ntt(self, u, log_n2, root, gen):
        assert u.numel() == 4 << log_n2
        self.torch.cuda.synchronize()
        self.gpu.ntt_device(u.data_ptr(), log_n2, root, coset_gen=gen)
        return u

    def equal(self, X, n1, j1, u):
        n2 = u.numel() // 4
        return self.torch.equal(X.view(n2, n1, 4)[:, j1], u.view(n2, 4))
