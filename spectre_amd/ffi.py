"""ctypes binding over libspectre_gpu.so (the product C ABI).

Mirrors include/spectre_gpu.h one-to-one. Compute entry points require a
visible AMD GPU; only the host-side reductions (`combine_partials`,
`combine_window_partials`, `msm_fold_window`), the pure tuning queries and
`version` work without one — exactly the contract of the C library.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SPECTRE_GPU_LIB overrides the library path (tuning-variant A/B builds)
_LIB = os.environ.get("SPECTRE_GPU_LIB",
                      os.path.join(_HERE, "libspectre_gpu.so"))

SCALARS_MONTGOMERY = 0
SCALARS_CANONICAL = 1
WINDOW_BITS = 16  # = SPECTRE_MSM_WINDOW_BITS
NUM_WINDOWS = 16  # = SPECTRE_MSM_NUM_WINDOWS
NUM_BUCKETS = NUM_WINDOWS * (1 << (WINDOW_BITS - 1))
PARTIALS_BYTES = NUM_WINDOWS * 96  # per-shard Jacobian window sums
MSM_ACC_THREADS = 256  # bucket-accumulate workgroup size
MSM_ACC_E_MIN = 8      # bounds of the auto entries-per-thread rule
MSM_ACC_E_MAX = 64     # (= MSM_ACC_E_MIN / MSM_ACC_E_MAX in csrc/internal.hpp)
MSM_ACC_TARGET_BLOCKS = 2  # accumulate blocks the rule aims at per CU
MSM_TAIL_CHUNK = 8  # = SPECTRE_MSM_TAIL_CHUNK: buckets per reduction chunk
MSM_TAIL_LO = 64    # = SPECTRE_MSM_TAIL_LO: columns of a window's chunk grid
# rows of that grid: chunks per window / columns
MSM_TAIL_HI = (1 << (WINDOW_BITS - 1)) // MSM_TAIL_CHUNK // MSM_TAIL_LO

_lib = None


def lib_path() -> str:
    return _LIB


def load_library() -> ctypes.CDLL:
    """dlopen the product library and declare signatures. Raises if missing —
    build with `make -C spectre_amd/csrc` (or __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise RuntimeError(
            f"libspectre_gpu.so not found at {_LIB}; run __graft_entry__.build()"
        )
    lib = ctypes.CDLL(_LIB)
    c = ctypes
    lib.spectre_gpu_init.restype = c.c_void_p
    lib.spectre_gpu_init.argtypes = [c.c_int, c.POINTER(c.c_int)]
    lib.spectre_gpu_destroy.argtypes = [c.c_void_p]
    lib.spectre_gpu_last_error.restype = c.c_char_p
    lib.spectre_gpu_version.restype = c.c_char_p
    lib.spectre_gpu_device_count.restype = c.c_int
    lib.spectre_gpu_device_count.argtypes = [c.c_void_p]
    lib.spectre_gpu_msm_g1.restype = c.c_int
    lib.spectre_gpu_msm_g1.argtypes = [
        c.c_void_p, c.c_uint64, c.c_void_p, c.c_void_p, c.c_uint64,
        c.c_uint32, c.c_int, c.c_void_p,
    ]
    lib.spectre_gpu_msm_g1_batch.restype = c.c_int
    lib.spectre_gpu_msm_g1_batch.argtypes = [
        c.c_void_p, c.c_uint64, c.c_void_p, c.c_void_p, c.c_uint32,
        c.c_uint64, c.c_uint32, c.c_void_p,
    ]
    lib.spectre_gpu_msm_g1_batch_device.restype = c.c_int
    lib.spectre_gpu_msm_g1_batch_device.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint64,
        c.c_uint32, c.c_void_p,
    ]
    lib.spectre_gpu_msm_g1_device.restype = c.c_int
    lib.spectre_gpu_msm_g1_device.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_uint64, c.c_uint32,
        c.c_void_p,
    ]
    lib.spectre_gpu_msm_g1_shard_device.restype = c.c_int
    lib.spectre_gpu_msm_g1_shard_device.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_uint64, c.c_uint32,
        c.c_void_p,
    ]
    lib.spectre_gpu_msm_g1_shard_device_timed.restype = c.c_int
    lib.spectre_gpu_msm_g1_shard_device_timed.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_uint64, c.c_uint32,
        c.c_void_p, c.POINTER(c.c_double),
    ]
    lib.spectre_gpu_msm_g1_shard_device_async.restype = c.c_int
    lib.spectre_gpu_msm_g1_shard_device_async.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_uint64, c.c_uint32,
        c.c_void_p, c.POINTER(c.c_int),
    ]
    lib.spectre_gpu_msm_slot_wait.restype = c.c_int
    lib.spectre_gpu_msm_slot_wait.argtypes = [c.c_void_p, c.c_int, c.c_int]
    lib.spectre_gpu_set_msm_acc_entries.restype = c.c_int
    lib.spectre_gpu_set_msm_acc_entries.argtypes = [c.c_void_p, c.c_uint32]
    lib.spectre_gpu_msm_acc_auto_entries.restype = c.c_uint32
    lib.spectre_gpu_msm_acc_auto_entries.argtypes = [
        c.c_uint64, c.c_uint32, c.c_uint32,
    ]
    lib.spectre_gpu_msm_fold_window.restype = c.c_int
    lib.spectre_gpu_msm_fold_window.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
    ]
    lib.spectre_gpu_msm_g1_shard_windows_device.restype = c.c_int
    lib.spectre_gpu_msm_g1_shard_windows_device.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_uint64, c.c_uint32,
        c.c_uint32, c.c_uint32, c.c_void_p,
    ]
    lib.spectre_gpu_msm_g1_shard_windows_device_async.restype = c.c_int
    lib.spectre_gpu_msm_g1_shard_windows_device_async.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_uint64, c.c_uint32,
        c.c_uint32, c.c_uint32, c.c_void_p, c.POINTER(c.c_int),
    ]
    lib.spectre_gpu_msm_g1_combine_windows.restype = c.c_int
    lib.spectre_gpu_msm_g1_combine_windows.argtypes = [
        c.c_void_p, c.c_uint32, c.c_void_p,
    ]
    lib.spectre_gpu_fr_gate_eval.restype = c.c_int
    lib.spectre_gpu_fr_gate_eval.argtypes = [
        c.c_void_p, c.c_int, c.POINTER(c.c_void_p), c.c_uint32, c.c_void_p,
        c.c_uint32, c.POINTER(c.c_uint32), c.c_uint32, c.c_uint64, c.c_uint32,
        c.c_void_p, c.c_void_p,
    ]
    lib.spectre_gpu_msm_g1_combine.restype = c.c_int
    lib.spectre_gpu_msm_g1_combine.argtypes = [c.c_void_p, c.c_uint32, c.c_void_p]
    lib.spectre_gpu_ntt_fr.restype = c.c_int
    lib.spectre_gpu_ntt_fr.argtypes = [
        c.c_void_p, c.c_void_p, c.c_uint32, c.c_void_p, c.c_int, c.c_void_p,
    ]
    lib.spectre_gpu_ntt_fr_device.restype = c.c_int
    lib.spectre_gpu_ntt_fr_device.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_uint32, c.c_void_p, c.c_int,
        c.c_void_p,
    ]
    lib.spectre_gpu_ntt_split.restype = c.c_uint32
    lib.spectre_gpu_ntt_split.argtypes = [
        c.c_uint32, c.c_int, c.POINTER(c.c_uint32),
    ]
    lib.spectre_gpu_ntt_fr_extend_device.restype = c.c_int
    lib.spectre_gpu_ntt_fr_extend_device.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_uint32, c.c_uint32, c.c_void_p,
        c.c_void_p, c.c_void_p,
    ]
    lib.spectre_gpu_fr_vec_mul_periodic.restype = c.c_int
    lib.spectre_gpu_fr_vec_mul_periodic.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_uint32, c.c_void_p,
        c.c_uint64,
    ]
    lib.spectre_gpu_fr_vec_op.restype = c.c_int
    lib.spectre_gpu_fr_vec_op.argtypes = [
        c.c_void_p, c.c_int, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p,
        c.c_void_p, c.c_uint64,
    ]
    lib.spectre_gpu_fr_batch_invert.restype = c.c_int
    lib.spectre_gpu_fr_batch_invert.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_uint64,
    ]
    lib.spectre_gpu_fr_grand_product.restype = c.c_int
    lib.spectre_gpu_fr_grand_product.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
        c.c_uint64, c.c_void_p,
    ]
    lib.spectre_gpu_set_fr_scan_tile.restype = c.c_int
    lib.spectre_gpu_set_fr_scan_tile.argtypes = [c.c_void_p, c.c_uint32]
    lib.spectre_gpu_fr_scan_tile_default.restype = c.c_uint32
    lib.spectre_gpu_fr_scan_tile_default.argtypes = []
    lib.spectre_gpu_fr_poly_eval.restype = c.c_int
    lib.spectre_gpu_fr_poly_eval.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint32,
        c.c_void_p,
    ]
    lib.spectre_gpu_fr_poly_div_linear.restype = c.c_int
    lib.spectre_gpu_fr_poly_div_linear.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint64,
        c.c_void_p,
    ]
    lib.spectre_gpu_fr_lincomb.restype = c.c_int
    lib.spectre_gpu_fr_lincomb.argtypes = [
        c.c_void_p, c.c_int, c.POINTER(c.c_void_p), c.c_void_p, c.c_uint32,
        c.c_void_p, c.c_uint64,
    ]
    lib.spectre_gpu_fr_poly_eval_batch.restype = c.c_int
    lib.spectre_gpu_fr_poly_eval_batch.argtypes = [
        c.c_void_p, c.c_int, c.POINTER(c.c_void_p), c.c_uint32, c.c_uint64,
        c.c_void_p, c.c_uint32, c.c_void_p,
    ]
    lib.spectre_gpu_fr_poly_div_roots.restype = c.c_int
    lib.spectre_gpu_fr_poly_div_roots.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_uint32, c.c_void_p,
        c.c_uint64, c.c_void_p,
    ]
    lib.spectre_gpu_fr_lookup_permute.restype = c.c_int
    lib.spectre_gpu_fr_lookup_permute.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
        c.c_uint64,
    ]
    lib.spectre_gpu_fr_powers.restype = c.c_int
    lib.spectre_gpu_fr_powers.argtypes = [
        c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint64,
    ]
    lib.spectre_gpu_fr_permutation_terms.restype = c.c_int
    lib.spectre_gpu_fr_permutation_terms.argtypes = [
        c.c_void_p, c.c_int, c.POINTER(c.c_void_p), c.POINTER(c.c_void_p),
        c.c_uint32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint64,
    ]
    lib.spectre_gpu_malloc.restype = c.c_int
    lib.spectre_gpu_malloc.argtypes = [c.c_void_p, c.c_int, c.c_size_t,
                                       c.POINTER(c.c_void_p)]
    lib.spectre_gpu_free.restype = c.c_int
    lib.spectre_gpu_free.argtypes = [c.c_void_p, c.c_int, c.c_void_p]
    lib.spectre_gpu_upload.restype = c.c_int
    lib.spectre_gpu_upload.argtypes = [c.c_void_p, c.c_int, c.c_void_p,
                                       c.c_void_p, c.c_size_t]
    lib.spectre_gpu_download.restype = c.c_int
    lib.spectre_gpu_download.argtypes = [c.c_void_p, c.c_int, c.c_void_p,
                                         c.c_void_p, c.c_size_t]
    lib.spectre_gpu_synchronize.restype = c.c_int
    lib.spectre_gpu_synchronize.argtypes = [c.c_void_p, c.c_int]
    _lib = lib
    return lib


def version() -> str:
    return load_library().spectre_gpu_version().decode()


def msm_acc_auto_entries(entries: int, cus: int, resident_blocks: int) -> int:
    """Host-only: the library's auto rule for sorted entries per bucket
    accumulate thread (see spectre_gpu_set_msm_acc_entries)."""
    return load_library().spectre_gpu_msm_acc_auto_entries(
        entries, cus, resident_blocks)


def msm_fold_window(p0: bytes, p1: bytes, p2: bytes) -> bytes:
    """Host-only: the library's fold of a window's three device partials
    (96-byte Jacobian each) into its window sum,
    p0 + MSM_TAIL_CHUNK * (p1 + MSM_TAIL_LO * p2)."""
    lib = load_library()
    assert len(p0) == len(p1) == len(p2) == 96
    bufs = [(ctypes.c_uint8 * 96).from_buffer_copy(p) for p in (p0, p1, p2)]
    out = (ctypes.c_uint8 * 96)()
    rc = lib.spectre_gpu_msm_fold_window(*bufs, out)
    if rc != 0:
        raise RuntimeError(f"msm_fold_window failed rc={rc}: "
                           f"{lib.spectre_gpu_last_error().decode()}")
    return bytes(out)


def fr_scan_tile_default() -> int:
    """Host-only: the built-in elements per workgroup tile of
    fr_batch_invert / fr_grand_product (see set_fr_scan_tile)."""
    return load_library().spectre_gpu_fr_scan_tile_default()


def ntt_split(log_n: int, force3: bool = False) -> tuple[int, ...]:
    """Host-only: the axis log sizes, in pass order, into which the library
    splits a 2^log_n NTT (force3: under SPECTRE_NTT_FORCE3). Empty for
    log_n == 0 and log_n > 28."""
    k = (ctypes.c_uint32 * 3)()
    count = load_library().spectre_gpu_ntt_split(log_n, 1 if force3 else 0, k)
    return tuple(k[:count])


def combine_window_partials(partials: bytes, nshards: int) -> bytes:
    """Host-only: concatenated rank-ordered DISJOINT window slices (shard i =
    NUM_WINDOWS/nshards consecutive windows) -> affine result."""
    lib = load_library()
    assert len(partials) == NUM_WINDOWS * 96
    buf = (ctypes.c_uint8 * len(partials)).from_buffer_copy(partials)
    out = (ctypes.c_uint8 * 64)()
    rc = lib.spectre_gpu_msm_g1_combine_windows(buf, nshards, out)
    if rc != 0:
        raise RuntimeError(f"combine_windows failed rc={rc}: "
                           f"{lib.spectre_gpu_last_error().decode()}")
    return bytes(out)


def combine_partials(partials: bytes, nshards: int) -> bytes:
    """Host-only: combine shard window partials (rank order) to affine."""
    lib = load_library()
    assert len(partials) == nshards * PARTIALS_BYTES
    buf = (ctypes.c_uint8 * len(partials)).from_buffer_copy(partials)
    out = (ctypes.c_uint8 * 64)()
    rc = lib.spectre_gpu_msm_g1_combine(buf, nshards, out)
    if rc != 0:
        raise RuntimeError(f"combine failed rc={rc}: "
                           f"{lib.spectre_gpu_last_error().decode()}")
    return bytes(out)


class SpectreGpu:
    """A context over one or more MI355X devices. Raises without a GPU."""

    def __init__(self, device_ids=None):
        self._lib = load_library()
        if device_ids is None:
            device_ids = [0]
        arr = (ctypes.c_int * len(device_ids))(*device_ids)
        self._ctx = self._lib.spectre_gpu_init(len(device_ids), arr)
        if not self._ctx:
            raise RuntimeError(
                "spectre_gpu_init failed (no AMD GPU?): "
                + self._lib.spectre_gpu_last_error().decode()
            )

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.spectre_gpu_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(
                f"{what} failed rc={rc}: "
                f"{self._lib.spectre_gpu_last_error().decode()}"
            )

    # ---- host-pointer API (the halo2 seam) ----
    def msm(self, bases: bytes | None, scalars: bytes, n: int,
            canonical: bool = True, num_gpus: int = 1,
            bases_id: int = 0) -> bytes:
        out = (ctypes.c_uint8 * 64)()
        # read-only args pass zero-copy (the C side never writes them)
        b = ctypes.cast(ctypes.c_char_p(bases), ctypes.c_void_p) if bases else None
        s = ctypes.cast(ctypes.c_char_p(scalars), ctypes.c_void_p)
        rc = self._lib.spectre_gpu_msm_g1(
            self._ctx, bases_id, b, s, n,
            SCALARS_CANONICAL if canonical else SCALARS_MONTGOMERY, num_gpus,
            out)
        self._check(rc, "msm_g1")
        return bytes(out)

    def msm_batch(self, bases: bytes | None, scalars: bytes, nbatch: int,
                  n: int, canonical: bool = True, bases_id: int = 0) -> list[bytes]:
        """nbatch MSMs over one shared base set (batch-major scalars)."""
        assert len(scalars) == nbatch * n * 32
        out = (ctypes.c_uint8 * (64 * nbatch))()
        b = ctypes.cast(ctypes.c_char_p(bases), ctypes.c_void_p) if bases else None
        s = ctypes.cast(ctypes.c_char_p(scalars), ctypes.c_void_p)
        rc = self._lib.spectre_gpu_msm_g1_batch(
            self._ctx, bases_id, b, s, nbatch, n,
            SCALARS_CANONICAL if canonical else SCALARS_MONTGOMERY, out)
        self._check(rc, "msm_g1_batch")
        raw = bytes(out)
        return [raw[64 * i:64 * (i + 1)] for i in range(nbatch)]

    def msm_batch_device(self, d_bases: int, d_scalars: int, nbatch: int,
                         n: int, canonical: bool = True,
                         dev: int = 0) -> list[bytes]:
        out = (ctypes.c_uint8 * (64 * nbatch))()
        rc = self._lib.spectre_gpu_msm_g1_batch_device(
            self._ctx, dev, ctypes.c_void_p(d_bases),
            ctypes.c_void_p(d_scalars), nbatch, n,
            SCALARS_CANONICAL if canonical else SCALARS_MONTGOMERY, out)
        self._check(rc, "msm_g1_batch_device")
        raw = bytes(out)
        return [raw[64 * i:64 * (i + 1)] for i in range(nbatch)]

    def ntt(self, data: bytes, log_n: int, omega: bytes, inverse: bool = False,
            coset_gen: bytes | None = None) -> bytes:
        assert log_n > 28 or len(data) == 32 << log_n, "data length != 32*2^log_n"
        buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
        om = (ctypes.c_uint8 * 32).from_buffer_copy(omega)
        cg = ((ctypes.c_uint8 * 32).from_buffer_copy(coset_gen)
              if coset_gen else None)
        rc = self._lib.spectre_gpu_ntt_fr(self._ctx, buf, log_n, om,
                                          1 if inverse else 0, cg)
        self._check(rc, "ntt_fr")
        return bytes(buf)

    # ---- device-resident API (device pointers, e.g. torch .data_ptr()) ----
    def msm_device(self, d_bases: int, d_scalars: int, n: int,
                   canonical: bool = True, dev: int = 0) -> bytes:
        out = (ctypes.c_uint8 * 64)()
        rc = self._lib.spectre_gpu_msm_g1_device(
            self._ctx, dev, ctypes.c_void_p(d_bases),
            ctypes.c_void_p(d_scalars), n,
            SCALARS_CANONICAL if canonical else SCALARS_MONTGOMERY, out)
        self._check(rc, "msm_g1_device")
        return bytes(out)

    def msm_shard_device(self, d_bases: int, d_scalars: int, n: int,
                         canonical: bool = True, dev: int = 0) -> bytes:
        out = (ctypes.c_uint8 * PARTIALS_BYTES)()
        rc = self._lib.spectre_gpu_msm_g1_shard_device(
            self._ctx, dev, ctypes.c_void_p(d_bases),
            ctypes.c_void_p(d_scalars), n,
            SCALARS_CANONICAL if canonical else SCALARS_MONTGOMERY, out)
        self._check(rc, "msm_g1_shard_device")
        return bytes(out)

    def msm_shard_device_async(self, d_bases: int, d_scalars: int, n: int,
                               canonical: bool = True, dev: int = 0):
        """Enqueue a full shard MSM on one of two per-device pipeline slots
        and return (partials_buffer, slot) WITHOUT synchronizing. Call
        msm_slot_wait(slot) before reading the buffer; keep the returned
        ctypes buffer referenced until then (async D2H writes into it)."""
        out = (ctypes.c_uint8 * PARTIALS_BYTES)()
        slot = ctypes.c_int(-1)
        rc = self._lib.spectre_gpu_msm_g1_shard_device_async(
            self._ctx, dev, ctypes.c_void_p(d_bases),
            ctypes.c_void_p(d_scalars), n,
            SCALARS_CANONICAL if canonical else SCALARS_MONTGOMERY, out,
            ctypes.byref(slot))
        self._check(rc, "msm_g1_shard_device_async")
        return out, slot.value

    def set_msm_acc_entries(self, e: int) -> None:
        """Fix the sorted entries per bucket-accumulate thread (a multiple
        of 4); 0 restores the per-call auto choice. Results do not change."""
        rc = self._lib.spectre_gpu_set_msm_acc_entries(self._ctx, e)
        self._check(rc, "set_msm_acc_entries")

    def msm_slot_wait(self, slot: int, dev: int = 0) -> None:
        rc = self._lib.spectre_gpu_msm_slot_wait(self._ctx, dev, slot)
        self._check(rc, "msm_slot_wait")

    def msm_shard_windows_device(self, d_bases: int, d_scalars: int, n: int,
                                 w_lo: int, w_cnt: int,
                                 canonical: bool = True,
                                 dev: int = 0) -> bytes:
        """Window-sharded shard: this rank's w_cnt windows over ALL n
        points (disjoint across ranks; exchange = pure allgather)."""
        out = (ctypes.c_uint8 * (96 * w_cnt))()
        rc = self._lib.spectre_gpu_msm_g1_shard_windows_device(
            self._ctx, dev, ctypes.c_void_p(d_bases),
            ctypes.c_void_p(d_scalars), n,
            SCALARS_CANONICAL if canonical else SCALARS_MONTGOMERY,
            w_lo, w_cnt, out)
        self._check(rc, "msm_g1_shard_windows_device")
        return bytes(out)

    def msm_shard_windows_device_async(self, d_bases: int, d_scalars: int,
                                       n: int, w_lo: int, w_cnt: int,
                                       canonical: bool = True, dev: int = 0):
        out = (ctypes.c_uint8 * (96 * w_cnt))()
        slot = ctypes.c_int(-1)
        rc = self._lib.spectre_gpu_msm_g1_shard_windows_device_async(
            self._ctx, dev, ctypes.c_void_p(d_bases),
            ctypes.c_void_p(d_scalars), n,
            SCALARS_CANONICAL if canonical else SCALARS_MONTGOMERY,
            w_lo, w_cnt, out, ctypes.byref(slot))
        self._check(rc, "msm_g1_shard_windows_device_async")
        return out, slot.value

    def msm_shard_device_timed(self, d_bases: int, d_scalars: int, n: int,
                               canonical: bool = True, dev: int = 0):
        """Returns (partials_bytes, stage_ms dict) — stage timings from HIP
        events on the library stream (see spectre_gpu.h)."""
        out = (ctypes.c_uint8 * PARTIALS_BYTES)()
        ms = (ctypes.c_double * 8)()
        rc = self._lib.spectre_gpu_msm_g1_shard_device_timed(
            self._ctx, dev, ctypes.c_void_p(d_bases),
            ctypes.c_void_p(d_scalars), n,
            SCALARS_CANONICAL if canonical else SCALARS_MONTGOMERY, out, ms)
        self._check(rc, "msm_g1_shard_device_timed")
        stages = dict(zip(
            ["digits", "sort", "offsets", "bucket_acc", "chunks", "reduce",
             "total", "real_entries"], list(ms)))
        return bytes(out), stages

    def ntt_device(self, d_data: int, log_n: int, omega: bytes,
                   inverse: bool = False, coset_gen: bytes | None = None,
                   dev: int = 0) -> None:
        om = (ctypes.c_uint8 * 32).from_buffer_copy(omega)
        cg = ((ctypes.c_uint8 * 32).from_buffer_copy(coset_gen)
              if coset_gen else None)
        rc = self._lib.spectre_gpu_ntt_fr_device(
            self._ctx, dev, ctypes.c_void_p(d_data), log_n, om,
            1 if inverse else 0, cg)
        self._check(rc, "ntt_fr_device")

    def ntt_extend_device(self, d_coeffs: int, log_n: int, ext_bits: int,
                          d_out: int, omega_ext: bytes,
                          coset_gen: bytes | None = None,
                          dev: int = 0) -> None:
        """halo2's coeff_to_extended: the forward (coset) NTT at
        2^(log_n + ext_bits), root omega_ext, of the 2^log_n coefficients at
        d_coeffs followed by zeros, into the 2^(log_n + ext_bits) elements at
        d_out. d_out may equal d_coeffs; the elements behind the coefficients
        are never read. Otherwise the two must not overlap."""
        om = (ctypes.c_uint8 * 32).from_buffer_copy(omega_ext)
        cg = ((ctypes.c_uint8 * 32).from_buffer_copy(coset_gen)
              if coset_gen else None)
        rc = self._lib.spectre_gpu_ntt_fr_extend_device(
            self._ctx, dev, ctypes.c_void_p(d_coeffs), log_n, ext_bits,
            ctypes.c_void_p(d_out), om, cg)
        self._check(rc, "ntt_fr_extend_device")

    # gate-expression evaluator opcodes (spectre_gpu.h)
    GATE_COL, GATE_CONST, GATE_ADD, GATE_SUB, GATE_MUL, GATE_NEG = range(6)

    def gate_eval(self, d_cols: list[int], constants: bytes,
                  program: list[tuple[int, int, int]], n: int,
                  rot_scale: int = 1, y: bytes | None = None,
                  d_out: int = 0, dev: int = 0) -> None:
        """Evaluate a gate expression over n rows into device buffer d_out
        (out = out*y + v when y is given). program = [(op, a, rot)]."""
        cols = (ctypes.c_void_p * len(d_cols))(*d_cols)
        prog = (ctypes.c_uint32 * (3 * len(program)))()
        for i, (op, a, b) in enumerate(program):
            prog[3 * i] = op
            prog[3 * i + 1] = a
            prog[3 * i + 2] = b & 0xFFFFFFFF
        con = ((ctypes.c_uint8 * len(constants)).from_buffer_copy(constants)
               if constants else None)
        yb = (ctypes.c_uint8 * 32).from_buffer_copy(y) if y else None
        rc = self._lib.spectre_gpu_fr_gate_eval(
            self._ctx, dev, cols, len(d_cols), con,
            len(constants) // 32, prog, len(program), n, rot_scale, yb,
            ctypes.c_void_p(d_out))
        self._check(rc, "fr_gate_eval")

    VEC_ADD, VEC_SUB, VEC_MUL, VEC_SCALE, VEC_ADD_SCALED = range(5)

    def fr_vec_op(self, op: int, d_a: int, d_b: int | None, c: bytes | None,
                  d_out: int, n: int, dev: int = 0) -> None:
        """Pointwise Fr vector op on device buffers (Montgomery form)."""
        cc = (ctypes.c_uint8 * 32).from_buffer_copy(c) if c else None
        rc = self._lib.spectre_gpu_fr_vec_op(
            self._ctx, dev, op, ctypes.c_void_p(d_a),
            ctypes.c_void_p(d_b) if d_b else None, cc,
            ctypes.c_void_p(d_out), n)
        self._check(rc, "fr_vec_op")

    VEC_PERIOD_MAX = 64  # = SPECTRE_VEC_PERIOD_MAX

    def fr_vec_mul_periodic(self, d_a: int, table: bytes, d_out: int, n: int,
                            dev: int = 0) -> None:
        """d_out[i] = d_a[i] * table[i mod period] over n Montgomery Fr
        elements (halo2's divide_by_vanishing_poly with table =
        t_evaluations); period = len(table) / 32, a power of two up to
        VEC_PERIOD_MAX. d_out may equal d_a."""
        assert len(table) % 32 == 0
        tab = (ctypes.c_uint8 * max(32, len(table))).from_buffer_copy(
            table.ljust(32, b"\0"))
        rc = self._lib.spectre_gpu_fr_vec_mul_periodic(
            self._ctx, dev, ctypes.c_void_p(d_a), tab, len(table) // 32,
            ctypes.c_void_p(d_out), n)
        self._check(rc, "fr_vec_mul_periodic")

    def fr_batch_invert(self, d_in: int, d_out: int, n: int,
                        dev: int = 0) -> None:
        """d_out[i] = d_in[i]^-1 over n Montgomery Fr elements; zero stays
        zero. d_out may equal d_in."""
        rc = self._lib.spectre_gpu_fr_batch_invert(
            self._ctx, dev, ctypes.c_void_p(d_in), ctypes.c_void_p(d_out), n)
        self._check(rc, "fr_batch_invert")

    def fr_grand_product(self, d_num: int, d_den: int | None,
                         z0: bytes | None, d_z: int, n: int,
                         dev: int = 0) -> bytes:
        """d_z[i] = z0 * prod_{j<i} num[j] / den[j] for i < n (d_den None: no
        denominators; z0 None: one). Returns the i = n value, which seeds the
        next chunk. d_z may equal d_num or d_den."""
        seed = (ctypes.c_uint8 * 32).from_buffer_copy(z0) if z0 else None
        last = (ctypes.c_uint8 * 32)()
        rc = self._lib.spectre_gpu_fr_grand_product(
            self._ctx, dev, ctypes.c_void_p(d_num),
            ctypes.c_void_p(d_den) if d_den else None, seed,
            ctypes.c_void_p(d_z), n, last)
        self._check(rc, "fr_grand_product")
        return bytes(last)

    def set_fr_scan_tile(self, elems: int) -> None:
        """Fix the elements per workgroup tile of the two calls above (a
        multiple of 256 up to fr_scan_tile_default()); 0 restores the
        default. Results do not change."""
        rc = self._lib.spectre_gpu_set_fr_scan_tile(self._ctx, elems)
        self._check(rc, "set_fr_scan_tile")

    POLY_EVAL_MAX_POINTS = 8  # = SPECTRE_POLY_EVAL_MAX_POINTS

    def fr_poly_eval(self, d_coeffs: int, n: int, points: list[bytes],
                     dev: int = 0) -> list[bytes]:
        """[sum_i d_coeffs[i] * x^i for x in points] over n Montgomery Fr
        coefficients on the device, read once for all of the 1..8 points."""
        assert all(len(p) == 32 for p in points)
        npts = len(points)
        raw = b"".join(points)
        pts = (ctypes.c_uint8 * max(32, len(raw))).from_buffer_copy(
            raw.ljust(32, b"\0"))
        out = (ctypes.c_uint8 * max(32, 32 * npts))()
        rc = self._lib.spectre_gpu_fr_poly_eval(
            self._ctx, dev, ctypes.c_void_p(d_coeffs), n, pts, npts, out)
        self._check(rc, "fr_poly_eval")
        raw = bytes(out)
        return [raw[32 * i:32 * (i + 1)] for i in range(npts)]

    def fr_poly_div_linear(self, d_a: int, z: bytes, d_q: int, n: int,
                           dev: int = 0) -> bytes:
        """d_q[i] = sum_{j>i} d_a[j] * z^(j-i-1) for i < n, the quotient of
        a(X) by (X - z) (d_q[:n-1] is halo2's kate_division, d_q[n-1] = 0).
        Returns the remainder a(z). d_q may equal d_a."""
        zz = (ctypes.c_uint8 * 32).from_buffer_copy(z)
        rem = (ctypes.c_uint8 * 32)()
        rc = self._lib.spectre_gpu_fr_poly_div_linear(
            self._ctx, dev, ctypes.c_void_p(d_a), zz, ctypes.c_void_p(d_q), n,
            rem)
        self._check(rc, "fr_poly_div_linear")
        return bytes(rem)

    OPEN_MAX_POLYS = 32  # = SPECTRE_OPEN_MAX_POLYS

    def fr_lincomb(self, d_polys: list[int], coeffs: list[bytes], d_out: int,
                   n: int, dev: int = 0) -> None:
        """d_out[i] = sum_k coeffs[k] * d_polys[k][i] for i < n over
        Montgomery Fr, m = len(d_polys) in 1..OPEN_MAX_POLYS. d_out may equal
        any input and a pointer may be listed several times (the accumulator
        with coefficient one chains past OPEN_MAX_POLYS); any other overlap of
        d_out with an input is refused."""
        assert len(coeffs) == len(d_polys)
        assert all(len(c) == 32 for c in coeffs)
        m = len(d_polys)
        ptrs = (ctypes.c_void_p * max(1, m))(*d_polys)
        raw = b"".join(coeffs)
        cc = (ctypes.c_uint8 * max(32, len(raw))).from_buffer_copy(
            raw.ljust(32, b"\0"))
        rc = self._lib.spectre_gpu_fr_lincomb(
            self._ctx, dev, ptrs, cc, m,
            ctypes.c_void_p(d_out) if d_out else None, n)
        self._check(rc, "fr_lincomb")

    def fr_poly_eval_batch(self, d_polys: list[int], n: int,
                           points: list[bytes],
                           dev: int = 0) -> list[list[bytes]]:
        """out[k][p] = sum_i d_polys[k][i] * points[p]^i: the m =
        len(d_polys) polynomials (1..OPEN_MAX_POLYS, n Montgomery Fr
        coefficients each) of one rotation set at its 1..8 points, each
        polynomial read once, one synchronization."""
        assert all(len(p) == 32 for p in points)
        m, npts = len(d_polys), len(points)
        ptrs = (ctypes.c_void_p * max(1, m))(*d_polys)
        raw = b"".join(points)
        pts = (ctypes.c_uint8 * max(32, len(raw))).from_buffer_copy(
            raw.ljust(32, b"\0"))
        out = (ctypes.c_uint8 * max(32, 32 * m * npts))()
        rc = self._lib.spectre_gpu_fr_poly_eval_batch(
            self._ctx, dev, ptrs, m, n, pts, npts, out)
        self._check(rc, "fr_poly_eval_batch")
        raw = bytes(out)
        return [[raw[32 * (k * npts + p):32 * (k * npts + p + 1)]
                 for p in range(npts)] for k in range(m)]

    def fr_poly_div_roots(self, d_a: int, roots: list[bytes], d_q: int,
                          n: int, want_rems: bool = True,
                          dev: int = 0) -> list[bytes] | None:
        """fr_poly_div_linear by each of the 1..8 roots in turn with one
        synchronization: d_a -> d_q, then in place in d_q, which ends up
        holding the quotient of a by Z = prod (X - roots[j]) (its top
        min(len(roots), n) elements zero). Returns the remainders, which are
        the Newton coefficients of a mod Z over the roots in order
        (want_rems False: passes NULL and returns None). d_q may equal
        d_a."""
        assert all(len(z) == 32 for z in roots)
        nroots = len(roots)
        raw = b"".join(roots)
        zz = (ctypes.c_uint8 * max(32, len(raw))).from_buffer_copy(
            raw.ljust(32, b"\0"))
        rems = (ctypes.c_uint8 * max(32, 32 * nroots))() if want_rems else None
        rc = self._lib.spectre_gpu_fr_poly_div_roots(
            self._ctx, dev, ctypes.c_void_p(d_a), zz, nroots,
            ctypes.c_void_p(d_q), n, rems)
        self._check(rc, "fr_poly_div_roots")
        if rems is None:
            return None
        raw = bytes(rems)
        return [raw[32 * j:32 * (j + 1)] for j in range(nroots)]

    ERR_LOOKUP_MISS = -5  # = SPECTRE_ERR_LOOKUP_MISS

    def fr_lookup_permute(self, d_input: int, d_table: int, d_input_perm: int,
                          d_table_perm: int, u: int, dev: int = 0) -> None:
        """halo2's permute_expression_pair over u rows of Montgomery Fr on
        the device: d_input_perm = d_input sorted by canonical value,
        d_table_perm = d_table rearranged so that every row equals its input
        row or the input row repeats the one above. The four buffers must not
        overlap. An input value absent from the table raises with rc=-5."""
        rc = self._lib.spectre_gpu_fr_lookup_permute(
            self._ctx, dev, ctypes.c_void_p(d_input), ctypes.c_void_p(d_table),
            ctypes.c_void_p(d_input_perm), ctypes.c_void_p(d_table_perm), u)
        self._check(rc, "fr_lookup_permute")

    PERM_MAX_COLS = 8  # = SPECTRE_PERM_MAX_COLS

    def fr_powers(self, c: bytes | None, g: bytes, d_out: int, n: int,
                  dev: int = 0) -> None:
        """d_out[i] = c * g^i for i < n (c None: one) over Montgomery Fr; c
        and g are any field elements. With c = zeta and g = omega_ext this is
        the X column of the extended-domain permutation constraint."""
        cc = (ctypes.c_uint8 * 32).from_buffer_copy(c) if c else None
        gg = (ctypes.c_uint8 * 32).from_buffer_copy(g)
        rc = self._lib.spectre_gpu_fr_powers(
            self._ctx, dev, cc, gg, ctypes.c_void_p(d_out) if d_out else None,
            n)
        self._check(rc, "fr_powers")

    def fr_permutation_terms(self, d_values: list[int], d_sigmas: list[int],
                             beta: bytes, gamma: bytes, omega: bytes,
                             delta0: bytes | None, delta: bytes, d_num: int,
                             d_den: int, n: int, dev: int = 0) -> None:
        """One chunk of halo2's permutation::prover::commit over rows 0..n of
        m = len(d_values) columns (1..PERM_MAX_COLS):
          d_den[i] = prod_j (values[j][i] + beta*sigmas[j][i] + gamma)
          d_num[i] = prod_j (values[j][i] + beta*delta0*delta^j*omega^i + gamma)
        delta0 None: one. fr_grand_product(d_num, d_den, z0) then gives the
        chunk's Z column. The outputs must overlap nothing."""
        assert len(d_values) == len(d_sigmas)
        m = len(d_values)
        vals = (ctypes.c_void_p * max(1, m))(*d_values)
        sigs = (ctypes.c_void_p * max(1, m))(*d_sigmas)
        b, gm, w, d = ((ctypes.c_uint8 * 32).from_buffer_copy(x)
                       for x in (beta, gamma, omega, delta))
        d0 = (ctypes.c_uint8 * 32).from_buffer_copy(delta0) if delta0 else None
        rc = self._lib.spectre_gpu_fr_permutation_terms(
            self._ctx, dev, vals, sigs, m, b, gm, w, d0, d,
            ctypes.c_void_p(d_num) if d_num else None,
            ctypes.c_void_p(d_den) if d_den else None, n)
        self._check(rc, "fr_permutation_terms")

    # ---- device memory helpers ----
    def malloc(self, nbytes: int, dev: int = 0) -> int:
        p = ctypes.c_void_p()
        self._check(self._lib.spectre_gpu_malloc(self._ctx, dev, nbytes,
                                                 ctypes.byref(p)), "malloc")
        return p.value

    def free(self, d_ptr: int, dev: int = 0) -> None:
        self._check(self._lib.spectre_gpu_free(self._ctx, dev,
                                               ctypes.c_void_p(d_ptr)), "free")

    def upload(self, d_dst: int, data: bytes, dev: int = 0) -> None:
        buf = ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p)
        self._check(self._lib.spectre_gpu_upload(self._ctx, dev,
                                                 ctypes.c_void_p(d_dst), buf,
                                                 len(data)), "upload")

    def download(self, d_src: int, nbytes: int, dev: int = 0) -> bytes:
        buf = (ctypes.c_uint8 * nbytes)()
        self._check(self._lib.spectre_gpu_download(self._ctx, dev, buf,
                                                   ctypes.c_void_p(d_src),
                                                   nbytes), "download")
        return bytes(buf)

    def synchronize(self, dev: int = 0) -> None:
        self._check(self._lib.spectre_gpu_synchronize(self._ctx, dev), "sync")
