"""Integer reference of the multiopen calls (spectre_gpu_fr_lincomb,
spectre_gpu_fr_poly_eval_batch, spectre_gpu_fr_poly_div_roots) and of the
two-set opening they close: plain Python integers mod the BN254 scalar field
over tests/golden/bn254_ref.py, loaded by path. Polynomials are coefficient
lists, lowest degree first. Not a test module; tests/test_multiopen_ref.py
pins it and tests/test_multiopen_gpu.py compares the device with it."""
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "bn254_ref", os.path.join(HERE, "golden", "bn254_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
R = ref.R
MONT_INV = pow(ref.MONT, -1, R)


def ints(data: bytes) -> list[int]:
    return [int.from_bytes(data[i:i + 32], "little") * MONT_INV % R
            for i in range(0, len(data), 32)]


def enc(v: int) -> bytes:
    return ref.to_mont_bytes(v % R, R)


def mont(vals) -> bytes:
    return b"".join(enc(v) for v in vals)


def lincomb(polys, coeffs, n: int) -> list[int]:
    """out[i] = sum_k coeffs[k] * polys[k][i] for i < n."""
    assert len(polys) == len(coeffs)
    return [sum(c * p[i] for c, p in zip(coeffs, polys)) % R
            for i in range(n)]


def horner(a, x: int) -> int:
    s = 0
    for c in reversed(a):
        s = (s * x + c) % R
    return s


def div_linear(a, z: int):
    """(q, rem) with a(X) = (X - z) q(X) + rem and len(q) == len(a), so that
    q[len(a) - 1] == 0: spectre_gpu_fr_poly_div_linear."""
    q = [0] * len(a)
    for i in range(len(a) - 2, -1, -1):
        q[i] = (a[i + 1] + z * q[i + 1]) % R
    rem = (a[0] + z * q[0]) % R if a else 0
    return q, rem


def div_roots(a, roots):
    """div_linear by every root in turn: (q, rems), len(q) == len(a)."""
    q, rems = list(a), []
    for z in roots:
        q, rem = div_linear(q, z)
        rems.append(rem)
    return q, rems


def poly_mul(a, b) -> list[int]:
    if not a or not b:
        return []
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % R
    return out


def poly_add(a, b) -> list[int]:
    n = max(len(a), len(b))
    a = list(a) + [0] * (n - len(a))
    b = list(b) + [0] * (n - len(b))
    return [(x + y) % R for x, y in zip(a, b)]


def vanishing(roots) -> list[int]:
    """prod (X - z), expanded (monic, len(roots) + 1 coefficients)."""
    z_s = [1]
    for z in roots:
        z_s = poly_mul(z_s, [(-z) % R, 1])
    return z_s


def newton(rems, roots) -> list[int]:
    """sum_j rems[j] * prod_{i<j} (X - roots[i]), expanded."""
    out, basis = [], [1]
    for rem, z in zip(rems, roots):
        out = poly_add(out, [rem * b % R for b in basis])
        basis = poly_mul(basis, [(-z) % R, 1])
    return out


def newton_from_evals(roots, evals) -> list[int]:
    """Newton coefficients (divided differences) of the interpolant through
    (roots[j], evals[j]); the roots are distinct."""
    c = [e % R for e in evals]
    for lvl in range(1, len(roots)):
        for j in range(len(roots) - 1, lvl - 1, -1):
            c[j] = (c[j] - c[j - 1]) * pow(roots[j] - roots[j - lvl], -1, R) % R
    return c


def schoolbook_divmod(a, d):
    """(q, r) with a = d q + r and deg r < deg d, d monic; a trimmed of
    nothing: len(q) == max(len(a) - deg d, 0), len(r) == deg d."""
    assert d and d[-1] == 1
    deg = len(d) - 1
    r = list(a)
    q = [0] * max(len(a) - deg, 0)
    for i in range(len(a) - 1, deg - 1, -1):
        t = r[i]
        q[i - deg] = t
        if t:
            for j in range(deg + 1):
                r[i - deg + j] = (r[i - deg + j] - t * d[j]) % R
    r = (r + [0] * deg)[:deg]
    return q, r


def trim(a) -> list[int]:
    a = list(a)
    while a and a[-1] == 0:
        a.pop()
    return a


def shplonk_open(sets, y: int, v: int, u: int, n: int):
    """The algebra of one SHPLONK opening in integers. sets = [(points,
    polys)], every poly n coefficients; T = the union of the point sets in
    order of first appearance. With f_i = sum_k y^k p_{i,k}, r_i = f_i mod
    Z_{S_i}, n_i = (f_i - r_i) / Z_{S_i}:
      h = sum_i v^i n_i
      L = sum_i v^i Z_{T \\ S_i}(u) (f_i - r_i(u)) - Z_T(u) h
      W = L / (X - u), remainder zero.
    Returns a dict with f, quot (n_i, n elements), rems (Newton form of
    r_i over S_i in order), h, L, W (n elements each), and the scalars
    zdiff[i] = Z_{T \\ S_i}(u), r_u[i] = r_i(u), z_t = Z_T(u)."""
    t_pts = []
    for pts, _ in sets:
        for x in pts:
            if x not in t_pts:
                t_pts.append(x)
    z_t = horner(vanishing(t_pts), u)
    out = {"f": [], "quot": [], "rems": [], "zdiff": [], "r_u": [],
           "z_t": z_t}
    for pts, polys in sets:
        f = lincomb(polys, [pow(y, k, R) for k in range(len(polys))], n)
        q, rems = div_roots(f, pts)
        out["f"].append(f)
        out["quot"].append(q)
        out["rems"].append(rems)
        out["zdiff"].append(
            horner(vanishing([x for x in t_pts if x not in pts]), u))
        out["r_u"].append(horner(newton(rems, pts), u))
    vi = [pow(v, i, R) for i in range(len(sets))]
    out["h"] = lincomb(out["quot"], vi, n)
    coeffs = [vi[i] * out["zdiff"][i] for i in range(len(sets))]
    big_l = lincomb(out["f"] + [out["h"]], coeffs + [-z_t], n)
    big_l[0] = (big_l[0] - sum(c * r for c, r in zip(coeffs, out["r_u"]))) % R
    out["L"] = big_l
    out["W"], out["W_rem"] = div_linear(big_l, u)
    return out
