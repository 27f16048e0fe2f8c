#!/usr/bin/env python3
"""Opening-phase timing (GPU box): fr_poly_eval at 1, 4 and 8 points and
fr_poly_div_linear out of place and in place, on device buffers of 2^16,
2^20, 2^22 and 2^24 coefficients. The yardstick is fr_vec_op(SCALE) at the
same n from the same library: a streaming kernel that reads and writes every
element once and does one multiply per element. Each call's time is also
reported as a ratio to it.

Every timed call ends in the library's stream synchronize, so a host clock
around it is the call time. Warm-up calls come first (code-object load and
scratch allocation), then REPS timed calls; the median and the min..max
spread are reported. Writes one JSON file (default
profiles/opening_bench.json) and prints it. Not part of the bench contract
and not run by the test suite."""
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
from spectre_amd import SpectreGpu, ffi  # noqa: E402

WARMUP = 3
REPS = 20
POINT_COUNTS = (1, 4, 8)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def level_sizes(n, tile, stop, min_levels):
    """The partial vectors above n elements (poly_levels of the library)."""
    sizes, m = [], n
    while m > stop or len(sizes) < min_levels:
        m = -(-m // tile)
        sizes.append(m)
    return sizes


def eval_cost(n, tile, npoints):
    """(elements moved, multiplies) of one fr_poly_eval call, counted from
    poly.hip: a tile pass reads its vector and writes one partial per tile
    and point, and spends tile - 1 multiplies per tile and point (e - 1
    Horner steps per thread, 255 tree nodes)."""
    moved, muls, m = 0, 0, n
    for lvl, size in enumerate(level_sizes(n, tile, 1, 1)):
        moved += (m if lvl == 0 else npoints * m) + npoints * size
        muls += npoints * size * (tile - 1)
        m = size
    return moved, muls


def div_cost(n, tile):
    """(elements moved, multiplies) of one fr_poly_div_linear call: a tile
    pass per level below the top as above, then per level a scan that reads
    its vector and a seed per tile, writes the quotient, and spends
    2 (tile - 1) multiplies per tile (Horner and up-sweep, down-sweep and
    the per-thread recurrence)."""
    sizes = [n] + level_sizes(n, tile, tile, 0)
    moved = muls = 0
    for lvl, m in enumerate(sizes):
        tiles = -(-m // tile)
        if lvl + 1 < len(sizes):
            moved += m + tiles
            muls += tiles * (tile - 1)
            moved += tiles  # seeds
        moved += 2 * m
        muls += 2 * tiles * (tile - 1)
    return moved, muls


def entry(ms, n, moved, muls, scale_s):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "reps": len(ms),
            "gb_per_s": round(32 * moved / (med / 1e3) / 1e9, 1),
            "muls_per_element": round(muls / n, 4),
            "ratio_to_scale": round(med / 1e3 / scale_s, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log_sizes", nargs="*", type=int,
                    default=[16, 20, 22, 24])
    ap.add_argument("--out", default=os.path.join(HERE, "profiles",
                                                  "opening_bench.json"))
    args = ap.parse_args()
    gpu = SpectreGpu([0])
    tile = ffi.fr_scan_tile_default()
    base = 1 << 16
    a0 = oracle.gen_fr_vector(base, 21)
    pts = [a0[32 * i:32 * i + 32] for i in range(9)]
    z, c = pts[8], pts[0]
    results = []
    for log_n in args.log_sizes:
        n = 1 << log_n
        a = a0 * max(1, n // base)
        d_a, d_q = gpu.malloc(32 * n), gpu.malloc(32 * n)
        gpu.upload(d_a, a[:32 * n])
        calls = {"scale": lambda: gpu.fr_vec_op(gpu.VEC_SCALE, d_a, None, c,
                                                d_q, n)}
        for k in POINT_COUNTS:
            calls[f"eval_{k}"] = \
                lambda k=k: gpu.fr_poly_eval(d_a, n, pts[:k])
        calls["div"] = lambda: gpu.fr_poly_div_linear(d_a, z, d_q, n)
        # runs last: it overwrites the coefficients with their quotient
        calls["div_in_place"] = \
            lambda: gpu.fr_poly_div_linear(d_a, z, d_a, n)
        ms = {}
        for name, fn in calls.items():
            timed(fn, WARMUP)
            ms[name] = timed(fn, REPS)
        for d in (d_a, d_q):
            gpu.free(d)
        scale_s = statistics.median(ms["scale"]) / 1e3
        row = {"log_n": log_n,
               "scale": entry(ms["scale"], n, 2 * n, n, scale_s)}
        for k in POINT_COUNTS:
            row[f"eval_{k}"] = entry(ms[f"eval_{k}"], n,
                                     *eval_cost(n, tile, k), scale_s)
        for name in ("div", "div_in_place"):
            row[name] = entry(ms[name], n, *div_cost(n, tile), scale_s)
        results.append(row)
    gpu.close()
    doc = {"tool": "opening_bench", "tile": tile, "warmup": WARMUP,
           "note": "gb_per_s counts the 32 B elements each call reads and "
                   "writes, partial vectors included; ratio_to_scale is the "
                   "median over the median of fr_vec_op(SCALE) at the same n",
           "results": results}
    text = json.dumps(doc, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
