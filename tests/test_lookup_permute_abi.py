"""Lookup-permutation C-ABI checks that run WITHOUT a GPU: the library exports
the entry point, the header declares it and its miss code, and the Python
mirror has the method. No compute entry point is called here."""
import os

SYMBOL = "spectre_gpu_fr_lookup_permute"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_symbol():
    from spectre_amd import ffi
    lib = ffi.load_library()
    assert hasattr(lib, SYMBOL), f"missing export {SYMBOL}"
    assert len(getattr(lib, SYMBOL).argtypes) == 7


def test_header_declares_the_symbol_and_the_miss_code():
    with open(os.path.join(REPO, "include", "spectre_gpu.h")) as f:
        header = f.read()
    assert SYMBOL + "(" in header, f"{SYMBOL} not declared in spectre_gpu.h"
    assert "#define SPECTRE_ERR_LOOKUP_MISS (-5)" in header


def test_python_mirror_has_the_method():
    from spectre_amd import SpectreGpu
    assert callable(getattr(SpectreGpu, "fr_lookup_permute"))
    assert SpectreGpu.ERR_LOOKUP_MISS == -5
