"""Multiopen C-ABI checks that run WITHOUT a GPU: the library exports the
linear combination, the batched evaluation and the division by a point set,
the header declares them and their constant, and the Python mirror has the
methods. No compute entry point is called here."""
import os

SYMBOLS = ["spectre_gpu_fr_lincomb", "spectre_gpu_fr_poly_eval_batch",
           "spectre_gpu_fr_poly_div_roots"]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_multiopen_symbols():
    from spectre_amd import ffi
    lib = ffi.load_library()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), f"missing export {sym}"


def test_header_declares_multiopen_symbols():
    with open(os.path.join(REPO, "include", "spectre_gpu.h")) as f:
        header = f.read()
    for sym in SYMBOLS:
        assert sym + "(" in header, f"{sym} not declared in spectre_gpu.h"
    assert "#define SPECTRE_OPEN_MAX_POLYS 32u" in header


def test_python_mirror_has_the_methods():
    from spectre_amd import SpectreGpu
    for name in ("fr_lincomb", "fr_poly_eval_batch", "fr_poly_div_roots"):
        assert callable(getattr(SpectreGpu, name))
    assert SpectreGpu.OPEN_MAX_POLYS == 32
