"""Permutation-argument C-ABI checks that run WITHOUT a GPU: the library
exports the row-powers / permutation-terms entry points, the header declares
them and the column limit, and the Python mirror has the methods. No compute
entry point is called here."""
import os

SYMBOLS = ["spectre_gpu_fr_powers", "spectre_gpu_fr_permutation_terms"]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header() -> str:
    with open(os.path.join(REPO, "include", "spectre_gpu.h")) as f:
        return f.read()


def test_library_exports_permutation_symbols():
    from spectre_amd import ffi
    lib = ffi.load_library()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), f"missing export {sym}"


def test_header_declares_what_the_library_exports():
    text = header()
    for sym in SYMBOLS:
        assert sym + "(" in text, f"{sym} not declared in spectre_gpu.h"


def test_header_defines_the_column_limit():
    from spectre_amd import SpectreGpu
    assert "#define SPECTRE_PERM_MAX_COLS 8u" in header()
    assert SpectreGpu.PERM_MAX_COLS == 8


def test_python_mirror_has_the_methods():
    from spectre_amd import SpectreGpu
    for name in ("fr_powers", "fr_permutation_terms"):
        assert callable(getattr(SpectreGpu, name))
