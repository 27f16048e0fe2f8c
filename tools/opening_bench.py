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
profiles/opening_bench.json) and prints it.

--multiopen times the set-level calls instead, each against the single calls
it replaces from the same library in the same process, alternating call by
call: fr_lincomb at m = 2, 8 and 32 against the SCALE + (m - 1) ADD_SCALED
chain, fr_poly_eval_batch of 16 polynomials at 1 and 4 points against 16
fr_poly_eval calls, fr_poly_div_roots at 4 roots against 4 fr_poly_div_linear
calls (default output profiles/multiopen_bench.json).

Not part of the bench contract and not run by the test suite."""
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


LINCOMB_M = (2, 8, 32)
BATCH_POLYS = 16
BATCH_POINTS = (1, 4)
DIV_ROOTS = 4


def alternating(new, base, reps):
    """WARMUP calls of each, then reps rounds of (new, base) back to back in
    one process, so both see the same machine state. Returns (new ms, base
    ms)."""
    timed(new, WARMUP)
    timed(base, WARMUP)
    t_new, t_base = [], []
    for _ in range(reps):
        t_new += timed(new, 1)
        t_base += timed(base, 1)
    return t_new, t_base


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4),
            "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def pair(t_new, t_base, extra=None):
    row = {"new": spread(t_new), "baseline": spread(t_base),
           "reps": len(t_new),
           "new_over_baseline": round(statistics.median(t_new) /
                                      statistics.median(t_base), 3)}
    row.update(extra or {})
    return row


def multiopen_row(gpu, log_n, a, pts):
    """The set-level calls against the single calls they replace, the same
    library and process, alternating. The m polynomials are made on the
    device from one upload (SCALE by different constants)."""
    n = 1 << log_n
    m_max = max(LINCOMB_M + (BATCH_POLYS,))
    d_polys = [gpu.malloc(32 * n) for _ in range(m_max)]
    d_out, d_q = gpu.malloc(32 * n), gpu.malloc(32 * n)
    gpu.upload(d_polys[0], a[:32 * n])
    consts = [a[32 * (16 + k):32 * (17 + k)] for k in range(m_max)]
    for k in range(1, m_max):
        gpu.fr_vec_op(gpu.VEC_SCALE, d_polys[0], None, consts[k], d_polys[k],
                      n)
    row = {"log_n": log_n}

    def chain(m):
        gpu.fr_vec_op(gpu.VEC_SCALE, d_polys[0], None, consts[0], d_out, n)
        for k in range(1, m):
            gpu.fr_vec_op(gpu.VEC_ADD_SCALED, d_out, d_polys[k], consts[k],
                          d_out, n)

    for m in LINCOMB_M:
        t_new, t_base = alternating(
            lambda m=m: gpu.fr_lincomb(d_polys[:m], consts[:m], d_out, n),
            lambda m=m: chain(m), REPS)
        med = statistics.median(t_new)
        row[f"lincomb_{m}"] = pair(t_new, t_base, {
            "traffic_ratio": round((m + 1) / (3 * m - 1), 3),
            "gb_per_s": round(32 * (m + 1) * n / (med / 1e3) / 1e9, 1)})
    for k in BATCH_POINTS:
        t_new, t_base = alternating(
            lambda k=k: gpu.fr_poly_eval_batch(d_polys[:BATCH_POLYS], n,
                                               pts[:k]),
            lambda k=k: [gpu.fr_poly_eval(d, n, pts[:k])
                         for d in d_polys[:BATCH_POLYS]], REPS)
        row[f"eval_batch_{BATCH_POLYS}x{k}"] = pair(t_new, t_base)

    def div_chain():
        gpu.fr_poly_div_linear(d_polys[0], pts[0], d_q, n)
        for z in pts[1:DIV_ROOTS]:
            gpu.fr_poly_div_linear(d_q, z, d_q, n)

    t_new, t_base = alternating(
        lambda: gpu.fr_poly_div_roots(d_polys[0], pts[:DIV_ROOTS], d_q, n),
        div_chain, REPS)
    row[f"div_roots_{DIV_ROOTS}"] = pair(t_new, t_base)
    for d in d_polys + [d_out, d_q]:
        gpu.free(d)
    return row


def main_multiopen(args):
    gpu = SpectreGpu([0])
    base = 1 << 16
    a0 = oracle.gen_fr_vector(base, 21)
    pts = [a0[32 * i:32 * i + 32] for i in range(8)]
    results = []
    for log_n in args.log_sizes:
        a = a0 * max(1, (1 << log_n) // base)
        results.append(multiopen_row(gpu, log_n, a, pts))
    gpu.close()
    doc = {"tool": "opening_bench --multiopen",
           "tile": ffi.fr_scan_tile_default(), "warmup": WARMUP,
           "note": "new = one set-level call, baseline = the single calls it "
                   "replaces (lincomb_m: SCALE + (m - 1) ADD_SCALED; "
                   "eval_batch_16xk: 16 fr_poly_eval at k points; "
                   "div_roots_4: 4 fr_poly_div_linear), same library and "
                   "process, alternating call by call; traffic_ratio = "
                   "(m + 1) / (3m - 1), the elements moved by one lincomb "
                   "over those of the chain; gb_per_s counts (m + 1) n "
                   "elements of 32 B",
           "results": results}
    text = json.dumps(doc, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log_sizes", nargs="*", type=int,
                    default=[16, 20, 22, 24])
    ap.add_argument("--multiopen", action="store_true",
                    help="time fr_lincomb, fr_poly_eval_batch and "
                         "fr_poly_div_roots against the single calls they "
                         "replace (default output "
                         "profiles/multiopen_bench.json)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(
            HERE, "profiles", "multiopen_bench.json" if args.multiopen
            else "opening_bench.json")
    if args.multiopen:
        return main_multiopen(args)
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
