"""ctypes access to the two probe libraries, and the XYZZ byte images.

TEST INFRASTRUCTURE for test_dot2_edges.py and test_xyzz_curve.py:
tests/probe/curve_probe.hip (ff_dot2, the g1x_* forms) and, for the Jacobian
forms and add(mul, mul), tests/probe/field_probe.hip. Both are built by
build() into spectre_amd/. A missing library fails the test; nothing skips.
"""
import ctypes
import os

import pytest

import edge_operands as eo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = b"\x5a"
P, MONT = eo.P, eo.MONT

# op codes of tests/probe/curve_probe.hip and tests/probe/field_probe.hip
CURVE_OPS = {"dot2": 0, "dot2chain": 1, "x_dbl": 16, "x_madd": 17,
             "x_add": 18, "x_to_jac": 19}
FIELD_OPS = {"mul": 0, "add": 2, "g1_dbl": 16, "g1_madd": 17, "g1_add": 18}
FIELD_CODE = {name: i for i, name in enumerate(eo.FIELDS)}

_libs = {}


def _lib(stem: str, prefix: str):
    if stem not in _libs:
        path = os.path.join(REPO, "spectre_amd", f"lib{stem}.so")
        if not os.path.exists(path):
            pytest.fail(f"{path} not found; run __graft_entry__.build()")
        lib = ctypes.CDLL(path)
        for where in ("host", "device"):
            fn = getattr(lib, f"{prefix}_{where}")
            fn.restype = ctypes.c_int
            fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                           ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64]
        _libs[stem] = lib
    return _libs[stem]


def _call(fn, code, field, a, b, out_elem, n):
    out = ctypes.create_string_buffer(FILL * (out_elem * (n + 1)),
                                      out_elem * (n + 1))
    rc = fn(code, FIELD_CODE[field], a, b, out, n)
    raw = out.raw
    assert raw[out_elem * n:] == FILL * out_elem, "wrote past n"
    return rc, raw[:out_elem * n]


def curve_call_rc(where, op, field, a, b, out_elem, n):
    fn = getattr(_lib("spectre_curveprobe", "curveprobe"), f"curveprobe_{where}")
    return _call(fn, CURVE_OPS.get(op, op), field, a, b, out_elem, n)


def curve_call(where, op, field, a, b, out_elem, n) -> bytes:
    rc, out = curve_call_rc(where, op, field, a, b, out_elem, n)
    assert rc == 0, f"curveprobe_{where}({op}, {field}) returned {rc}"
    return out


def field_call(where, op, field, a, b, out_elem, n) -> bytes:
    fn = getattr(_lib("spectre_ffprobe", "ffprobe"), f"ffprobe_{where}")
    rc, out = _call(fn, FIELD_OPS[op], field, a, b, out_elem, n)
    assert rc == 0, f"ffprobe_{where}({op}, {field}) returned {rc}"
    return out


# ------------------------------------------------------------- XYZZ images
def xyzz_bytes(pt, lam: int) -> bytes:
    """(lam^2 x, lam^3 y, lam^2, lam^3) as a 128-byte image; the identity is
    (lam^2, lam^3, 0, 0)."""
    x, y = pt if pt is not None else (1, 1)
    l2, l3 = lam * lam % P, pow(lam, 3, P)
    zz, zzz = (l2, l3) if pt is not None else (0, 0)
    return eo.imgs_bytes([eo.fq_img(l2 * x % P), eo.fq_img(l3 * y % P),
                          eo.fq_img(zz), eo.fq_img(zzz)])


def xyzz_to_affine(data: bytes):
    """A 128-byte XYZZ image -> affine canonical (x, y), None iff ZZ = 0.
    Every coordinate must be a reduced image, the identity has ZZZ = 0 too,
    and every other point ZZ^3 == ZZZ^2."""
    X, Y, ZZ, ZZZ = eo.imgs_from(data)
    assert X < P and Y < P and ZZ < P and ZZZ < P, "unreduced XYZZ coordinate"
    if ZZ == 0:
        assert ZZZ == 0, "identity with ZZZ != 0"
        return None
    minv = pow(MONT, -1, P)
    X, Y, ZZ, ZZZ = (v * minv % P for v in (X, Y, ZZ, ZZZ))
    assert pow(ZZ, 3, P) == ZZZ * ZZZ % P, "ZZ^3 != ZZZ^2"
    return (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)
