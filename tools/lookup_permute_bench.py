#!/usr/bin/env python3
"""Lookup-permutation timing (GPU box): fr_lookup_permute on device buffers
at u = 2^20, 2^22 and 2^23, for two key shapes, against the transfers alone of
the only alternative (download A and S, upload A' and S', through the
library's own helpers; the host path pays its sort and its serial map walk on
top).

  range  table = 0 .. 2^19-1 repeated to length, inputs drawn from it: the
         range-check lookups, 19-bit keys, one short sort pass per column
  full   random Fr table, inputs drawn from it: the theta-compressed lookups,
         four 64-bit limb passes per column

Every timed call ends in the library's stream synchronize, so a host clock
around it is the call time. Warm-up calls come first (code-object load and
scratch allocation), then REPS timed calls; the median and the min..max spread
are reported. Prints one JSON line. Not part of the bench contract."""
import argparse
import json
import os
import random
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
RANGE_BITS = 19
BLOCK = 1 << 12  # inputs are drawn block-wise: whole runs of table rows
# the BN254 scalar modulus and the Montgomery radix of the 32-byte images
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = 1 << 256


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


def range_table(u):
    """0 .. 2^19-1 as Montgomery Fr, repeated to u rows."""
    k = 1 << RANGE_BITS
    one = b"".join((i * MONT % R).to_bytes(32, "little") for i in range(k))
    return one * (u // k)


def full_table(u):
    """u random Fr elements."""
    return oracle.gen_fr_vector(u, 31)


def draw_inputs(table, u, seed):
    """u inputs, every one a table value: BLOCK-row runs of the table picked
    at random with repeats (so inputs repeat and table values stay unused)."""
    rng = random.Random(seed)
    nblk = u // BLOCK
    out = bytearray()
    for _ in range(nblk):
        o = 32 * BLOCK * rng.randrange(nblk)
        out += table[o:o + 32 * BLOCK]
    return bytes(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log_sizes", nargs="*", type=int, default=[20, 22, 23])
    ap.add_argument("--shapes", default="range,full",
                    help="comma-separated subset of range,full (one shape "
                         "per run under a kernel trace)")
    args = ap.parse_args()
    makers = {"range": range_table, "full": full_table}
    shapes = args.shapes.split(",")
    assert shapes and all(s in makers for s in shapes), args.shapes
    gpu = SpectreGpu([0])
    results = []
    for log_u in args.log_sizes:
        u = 1 << log_u
        row = {"log_u": log_u}
        d_a, d_s, d_ap, d_sp = (gpu.malloc(32 * u) for _ in range(4))
        for shape in shapes:
            table = makers[shape](u)
            inputs = draw_inputs(table, u, 41 + log_u)
            gpu.upload(d_a, inputs)
            gpu.upload(d_s, table)
            call = lambda: gpu.fr_lookup_permute(d_a, d_s, d_ap, d_sp, u)  # noqa: E731
            for _ in range(WARMUP):
                call()
            row[shape] = stats(timed(call, REPS))
        out_bytes = inputs  # any 32u bytes: the upload size is what counts

        def transfers():
            gpu.download(d_a, 32 * u)
            gpu.download(d_s, 32 * u)
            gpu.upload(d_ap, out_bytes)
            gpu.upload(d_sp, out_bytes)

        transfers()  # warm
        tr_ms = timed(transfers, TRANSFER_REPS)
        for d in (d_a, d_s, d_ap, d_sp):
            gpu.free(d)
        tr = statistics.median(tr_ms)
        row["host_path_transfers_only"] = stats(tr_ms)
        row["transfers_gb_per_s"] = round(4 * 32 * u / tr / 1e6, 2)
        for shape in shapes:
            row[shape + "_mrows_per_s"] = round(
                u / row[shape]["median_ms"] / 1e3, 1)
            row[shape + "_faster_than_transfers"] = \
                row[shape]["median_ms"] < tr
        results.append(row)
    gpu.close()
    print(json.dumps({
        "tool": "lookup_permute_bench",
        "shapes": {"range": "table 0..2^19-1 repeated, inputs drawn from it",
                   "full": "u random Fr, inputs drawn from it"},
        "yardstick": "download A, S + upload A', S' (no host sort or walk)",
        "results": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
