"""Opening-phase C-ABI checks that run WITHOUT a GPU: the library exports the
polynomial evaluation / (X - z) division entry points, the header declares
them and the Python mirror has the methods. No compute entry point is called
here."""
import os

SYMBOLS = ["spectre_gpu_fr_poly_eval", "spectre_gpu_fr_poly_div_linear"]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_opening_symbols():
    from spectre_amd import ffi
    lib = ffi.load_library()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), f"missing export {sym}"


def test_header_declares_opening_symbols():
    with open(os.path.join(REPO, "include", "spectre_gpu.h")) as f:
        header = f.read()
    for sym in SYMBOLS:
        assert sym + "(" in header, f"{sym} not declared in spectre_gpu.h"
    assert "#define SPECTRE_POLY_EVAL_MAX_POINTS 8u" in header


def test_python_mirror_has_the_methods():
    from spectre_amd import SpectreGpu
    for name in ("fr_poly_eval", "fr_poly_div_linear"):
        assert callable(getattr(SpectreGpu, name))
    assert SpectreGpu.POLY_EVAL_MAX_POINTS == 8
