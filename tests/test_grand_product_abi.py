"""Grand-product C-ABI checks that run WITHOUT a GPU: the library exports the
batch-invert / grand-product entry points and the host-only tile query
answers. No compute entry point is called here."""

SYMBOLS = [
    "spectre_gpu_fr_batch_invert", "spectre_gpu_fr_grand_product",
    "spectre_gpu_set_fr_scan_tile", "spectre_gpu_fr_scan_tile_default",
]


def test_library_exports_grand_product_symbols():
    from spectre_amd import ffi
    lib = ffi.load_library()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), f"missing export {sym}"


def test_scan_tile_default_is_a_multiple_of_the_block():
    from spectre_amd import ffi
    tile = ffi.fr_scan_tile_default()
    assert tile > 0 and tile % 256 == 0


def test_python_mirror_has_the_methods():
    from spectre_amd import SpectreGpu
    for name in ("fr_batch_invert", "fr_grand_product", "set_fr_scan_tile"):
        assert callable(getattr(SpectreGpu, name))


def test_header_declares_what_the_library_exports():
    import os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "spectre_gpu.h")) as f:
        header = f.read()
    for sym in SYMBOLS:
        assert sym + "(" in header, f"{sym} not declared in spectre_gpu.h"
