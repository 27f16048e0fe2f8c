"""Extended-domain C-ABI checks that run WITHOUT a GPU: the library exports
the zero-padded coset NTT and the periodic multiply, the header declares them
and the Python mirror has the methods. No compute entry point is called
here."""
import os

SYMBOLS = ["spectre_gpu_ntt_fr_extend_device",
           "spectre_gpu_fr_vec_mul_periodic"]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_extend_symbols():
    from spectre_amd import ffi
    lib = ffi.load_library()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), f"missing export {sym}"


def test_header_declares_extend_symbols():
    with open(os.path.join(REPO, "include", "spectre_gpu.h")) as f:
        header = f.read()
    for sym in SYMBOLS:
        assert sym + "(" in header, f"{sym} not declared in spectre_gpu.h"
    assert "#define SPECTRE_VEC_PERIOD_MAX 64u" in header


def test_python_mirror_has_the_methods():
    from spectre_amd import SpectreGpu
    for name in ("ntt_extend_device", "fr_vec_mul_periodic"):
        assert callable(getattr(SpectreGpu, name))
    assert SpectreGpu.VEC_PERIOD_MAX == 64
