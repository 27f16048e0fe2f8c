#!/usr/bin/env python3
"""Permutation-argument timing (GPU box): fr_powers at 2^20 and 2^22 and
fr_permutation_terms at m = 2 columns for 2^20, 2^22 and 2^23, on device
buffers, next to

  * fr_grand_product on the same n, re-measured in the same run: the scan the
    terms feed. An elementwise pass that is not clearly faster than that
    three-launch scan has a defect;
  * the transfers alone of the only alternative (download the m value
    columns, upload num and den, through the library's own helpers; the host
    path pays its CPU products on top);
  * the per-call build of the row-power tables. It has no entry point of its
    own, so it is measured as a difference: fr_powers over 4096 rows (the
    whole low table, 4096 chains of six multiplies, plus 16 workgroups of
    output) minus fr_powers over 1 row (the same two launches, the table
    builder k_pow_tables and k_fr_powers, and the synchronize; two table
    entries). Every larger call builds that same low table, and its n / 4096
    high entries in further workgroups of the builder's one launch. The NTT's
    per-call coset table is the same builder and the same launch.

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

WARMUP = 3
REPS = 20
TRANSFER_REPS = 5
M = 2  # columns per chunk (cs_degree - 2 of a degree-4 circuit)
# Multiplies per row (counted from perm.hip): omega^i 1, per column
# beta*sigma 1 and (beta*delta^j)*omega^i 1, and 2 per column after the first
# for the two running products.
MULS_TERMS = 1 + 2 * M + 2 * (M - 1)
MULS_POWERS = 1
# Bytes each call has to move per row (32 B elements).
BYTES_TERMS = (2 * M + 2) * 32   # read m values, m sigmas; write num, den
BYTES_POWERS = 32                # write out
BYTES_PRODUCT = 5 * 32           # as tools/grand_product_bench.py counts it


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


def measure(fn):
    for _ in range(WARMUP):
        fn()
    return timed(fn, REPS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--powers", nargs="*", type=int, default=[20, 22])
    ap.add_argument("--terms", nargs="*", type=int, default=[20, 22, 23])
    ap.add_argument("--label", default="",
                    help="recorded as given (the commit measured)")
    args = ap.parse_args()
    gpu = SpectreGpu([0])
    base = 1 << 16
    seeds = oracle.gen_fr_vector(base + 5, 21)
    col0 = [oracle.gen_fr_vector(base, 22 + k) for k in range(2 * M)]
    beta, gamma, omega, delta, zeta = (
        seeds[32 * (base + k):32 * (base + k + 1)] for k in range(5))

    # the table build, as the docstring defines it
    d_small = gpu.malloc(32 * 4096)
    floor_ms = measure(lambda: gpu.fr_powers(zeta, omega, d_small, 1))
    low_ms = measure(lambda: gpu.fr_powers(zeta, omega, d_small, 4096))
    gpu.free(d_small)
    build_ms = statistics.median(low_ms) - statistics.median(floor_ms)

    powers = []
    for log_n in args.powers:
        n = 1 << log_n
        d_out = gpu.malloc(32 * n)
        ms = measure(lambda: gpu.fr_powers(zeta, omega, d_out, n))
        gpu.free(d_out)
        s = statistics.median(ms) / 1e3
        powers.append({
            "log_n": log_n, "fr_powers": stats(ms),
            "gb_per_s": round(BYTES_POWERS * n / s / 1e9, 1),
            "table_build_share": round(build_ms / 1e3 / s, 4)})

    terms = []
    for log_n in args.terms:
        n = 1 << log_n
        reps = max(1, n // base)
        d_cols = [gpu.malloc(32 * n) for _ in range(2 * M)]
        for d, c in zip(d_cols, col0):
            gpu.upload(d, c * reps)
        d_num, d_den, d_z = (gpu.malloc(32 * n) for _ in range(3))
        t_ms = measure(lambda: gpu.fr_permutation_terms(
            d_cols[:M], d_cols[M:], beta, gamma, omega, None, delta, d_num,
            d_den, n))
        gp_ms = measure(
            lambda: gpu.fr_grand_product(d_num, d_den, None, d_z, n))
        host = col0[0] * reps

        def transfers():
            for d in d_cols[:M]:
                gpu.download(d, 32 * n)
            gpu.upload(d_num, host)
            gpu.upload(d_den, host)

        transfers()  # warm
        tr_ms = timed(transfers, TRANSFER_REPS)
        for d in d_cols + [d_num, d_den, d_z]:
            gpu.free(d)
        t_s = statistics.median(t_ms) / 1e3
        gp_s = statistics.median(gp_ms) / 1e3
        tr_s = statistics.median(tr_ms) / 1e3
        terms.append({
            "log_n": log_n, "m": M,
            "permutation_terms": stats(t_ms),
            "grand_product_same_n": stats(gp_ms),
            "host_path_transfers_only": stats(tr_ms),
            "terms_gb_per_s": round(BYTES_TERMS * n / t_s / 1e9, 1),
            "terms_gmul_per_s": round(MULS_TERMS * n / t_s / 1e9, 2),
            "grand_product_gb_per_s": round(BYTES_PRODUCT * n / gp_s / 1e9, 1),
            "transfers_gb_per_s": round((M + 2) * 32 * n / tr_s / 1e9, 2),
            "table_build_share": round(build_ms / 1e3 / t_s, 4),
            "terms_over_grand_product": round(t_s / gp_s, 3),
            "terms_faster_than_grand_product": t_s < gp_s,
            "device_faster_than_transfers": t_s < tr_s,
        })
    gpu.close()
    print(json.dumps({
        "tool": "permutation_bench",
        "label": args.label,
        "muls_per_row": {"fr_powers": MULS_POWERS,
                         "permutation_terms": MULS_TERMS},
        "bytes_per_row": {"fr_powers": BYTES_POWERS,
                          "permutation_terms": BYTES_TERMS,
                          "grand_product": BYTES_PRODUCT},
        "table_build": {
            "fr_powers_1_row": stats(floor_ms),
            "fr_powers_4096_rows": stats(low_ms),
            "difference_of_medians_ms": round(build_ms, 4),
            "note": "the launches and the synchronize are in both; the "
                    "difference is the 4096-entry low table and 16 "
                    "workgroups of output"},
        "powers": powers, "terms": terms}))
    ok = all(r["terms_faster_than_grand_product"]
             and r["device_faster_than_transfers"] for r in terms)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
