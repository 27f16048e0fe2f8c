#!/usr/bin/env python3
"""Grand-product timing (GPU box): fr_batch_invert and fr_grand_product on
device buffers at 2^20, 2^22 and 2^23, against the transfers alone of the
only alternative (download num and den, upload z, through the library's own
helpers; the host path pays its CPU inversion and serial product on top).

Every timed call ends in the library's stream synchronize, so a host clock
around it is the call time. Warm-up calls come first (code-object load and
scratch allocation), then REPS timed calls; the median and the min..max
spread are reported. Prints one JSON line. Not part of the bench contract."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "oracle"))
import pywrap as oracle  # noqa: E402
from spectre_amd import SpectreGpu  # noqa: E402

MUL_CEILING = 135e9  # asm Montgomery multiplies per second
WARMUP = 3
REPS = 20
TRANSFER_REPS = 5

# Multiplies the kernels issue per element at the default tile (4 elements
# per thread; counted from poly.hip), excluding the one Fermat inversion per
# workgroup. Per thread, batch invert: own prefixes 3, product tree up 1 and
# down 2, backward sweep 6 = 12. Grand product adds the ratio 4, the thread
# product 3 and its tree 1, and in the scan launch own prefixes 3, tree up 1
# and down 1, outputs 3 = 28.
MULS_INVERT = 12 / 4
MULS_PRODUCT = 28 / 4
# Bytes each call has to move per element (32 B elements).
BYTES_INVERT = 2 * 32        # read in, write out
BYTES_PRODUCT = 5 * 32       # read num, den; write r; read r; write z


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4),
            "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log_sizes", nargs="*", type=int, default=[20, 22, 23])
    args = ap.parse_args()
    gpu = SpectreGpu([0])
    base = 1 << 16
    num0 = oracle.gen_fr_vector(base, 11)
    den0 = oracle.gen_fr_vector(base, 12)
    results = []
    for log_n in args.log_sizes:
        n = 1 << log_n
        reps = max(1, n // base)
        num, den = num0 * reps, den0 * reps
        d_num, d_den, d_z = (gpu.malloc(32 * n) for _ in range(3))
        gpu.upload(d_num, num)
        gpu.upload(d_den, den)
        for _ in range(WARMUP):
            gpu.fr_batch_invert(d_den, d_z, n)
            gpu.fr_grand_product(d_num, d_den, None, d_z, n)
        inv_ms = timed(lambda: gpu.fr_batch_invert(d_den, d_z, n), REPS)
        gp_ms = timed(
            lambda: gpu.fr_grand_product(d_num, d_den, None, d_z, n), REPS)

        def transfers():
            gpu.download(d_num, 32 * n)
            gpu.download(d_den, 32 * n)
            gpu.upload(d_z, num)

        transfers()  # warm
        tr_ms = timed(transfers, TRANSFER_REPS)
        for d in (d_num, d_den, d_z):
            gpu.free(d)
        inv_s = statistics.median(inv_ms) / 1e3
        gp_s = statistics.median(gp_ms) / 1e3
        tr_s = statistics.median(tr_ms) / 1e3
        results.append({
            "log_n": log_n,
            "batch_invert": stats(inv_ms),
            "grand_product": stats(gp_ms),
            "host_path_transfers_only": stats(tr_ms),
            "batch_invert_gmul_per_s": round(MULS_INVERT * n / inv_s / 1e9, 2),
            "grand_product_gmul_per_s": round(MULS_PRODUCT * n / gp_s / 1e9, 2),
            "batch_invert_share_of_mul_ceiling":
                round(MULS_INVERT * n / inv_s / MUL_CEILING, 4),
            "grand_product_share_of_mul_ceiling":
                round(MULS_PRODUCT * n / gp_s / MUL_CEILING, 4),
            "batch_invert_gb_per_s": round(BYTES_INVERT * n / inv_s / 1e9, 1),
            "grand_product_gb_per_s": round(BYTES_PRODUCT * n / gp_s / 1e9, 1),
            "transfers_gb_per_s": round(3 * 32 * n / tr_s / 1e9, 2),
            "device_faster_than_transfers": gp_s < tr_s,
        })
    gpu.close()
    print(json.dumps({
        "tool": "grand_product_bench",
        "mul_ceiling_per_s": MUL_CEILING,
        "muls_per_element": {"batch_invert": MULS_INVERT,
                             "grand_product": MULS_PRODUCT},
        "bytes_per_element": {"batch_invert": BYTES_INVERT,
                              "grand_product": BYTES_PRODUCT},
        "note": "multiplies exclude the one Fermat inversion (~380 serial "
                "multiplies on one wave) per workgroup",
        "results": results}))
    return 0 if all(r["device_faster_than_transfers"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
