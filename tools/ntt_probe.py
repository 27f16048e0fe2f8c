#!/usr/bin/env python3
"""NTT timing probe (GPU box): device-resident forward/inverse/coset NTT at
the BASELINE sizes, and the zero-padded coset NTT (extend) from a quarter of
each size. Not part of the bench contract — a tuning tool."""
import argparse
import hashlib
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "oracle"))
import pywrap as oracle  # noqa: E402
from spectre_amd import SpectreGpu  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
EXT_BITS = 2  # the pinned circuits' extended_k - k


def omega_for(log_n):
    g7 = oracle.fr_from_canonical((7).to_bytes(32, "little"))
    w = oracle.fr_pow(g7, ((R - 1) >> 28).to_bytes(32, "little"))
    for _ in range(28 - log_n):
        w = oracle.fr_mul(w, w)
    return w


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("sizes", nargs="*", type=int, default=[20, 22, 23, 24],
                    metavar="LOG_N")
    ap.add_argument("--reps", default="10",
                    help="calls per timed window: one count, or one per "
                         "size separated by commas (default 10)")
    ap.add_argument("--hash", action="store_true",
                    help="also print the sha256 of the downloaded output of "
                         "one forward, one inverse, one coset and one "
                         "extend call per size, each on the freshly uploaded "
                         "input")
    args = ap.parse_args()
    reps_list = [int(r) for r in args.reps.split(",")]
    if len(reps_list) == 1:
        reps_list *= len(args.sizes)
    if len(reps_list) != len(args.sizes) or min(reps_list) < 1:
        ap.error("--reps wants one positive count, or one per size")

    gpu = SpectreGpu([0])
    g = oracle.fr_from_canonical((5).to_bytes(32, "little"))
    for log_n, reps in zip(args.sizes, reps_list):
        n = 1 << log_n
        data = oracle.gen_fr_vector(min(n, 1 << 20), 7)
        data = data * (n // (1 << min(log_n, 20)))
        w = omega_for(log_n)
        wi = oracle.fr_inv(w)
        legs = [("fwd", dict()), ("inv", dict(inverse=True)),
                ("coset", dict(coset_gen=g))]
        d = gpu.malloc(32 * n)
        if args.hash:
            for name, kw in legs:
                gpu.upload(d, data)
                gpu.ntt_device(d, log_n, wi if kw.get("inverse") else w, **kw)
                h = hashlib.sha256(gpu.download(d, 32 * n)).hexdigest()
                print(f"2^{log_n} {name} sha256 {h}")
        gpu.upload(d, data)
        gpu.ntt_device(d, log_n, w)  # warm (plan build)
        gpu.ntt_device(d, log_n, wi, inverse=True)
        for name, kw in legs:
            om = wi if kw.get("inverse") else w
            t0 = time.time()
            for _ in range(reps):
                gpu.ntt_device(d, log_n, om, **kw)
            dt = (time.time() - t0) / reps * 1e3
            gb = 2 * n * 32 / 1e9  # algorithmic: one read+write per pass pair
            print(f"2^{log_n} {name}: {dt:7.3f} ms  "
                  f"({2 * gb / dt * 1e3:7.1f} GB/s algorithmic 2-pass)"
                  f"  x{reps}")
        if log_n >= EXT_BITS:
            # extend: 2^(log_n - 2) coefficients -> the same 2^log_n coset
            # domain, in place; what a call leaves in the first quarter is
            # the next call's input
            if args.hash:
                gpu.upload(d, data[:32 * (n >> EXT_BITS)])
                gpu.ntt_extend_device(d, log_n - EXT_BITS, EXT_BITS, d, w,
                                      coset_gen=g)
                h = hashlib.sha256(gpu.download(d, 32 * n)).hexdigest()
                print(f"2^{log_n} extend sha256 {h}")
            gpu.ntt_extend_device(d, log_n - EXT_BITS, EXT_BITS, d, w,
                                  coset_gen=g)  # warm
            t0 = time.time()
            for _ in range(reps):
                gpu.ntt_extend_device(d, log_n - EXT_BITS, EXT_BITS, d, w,
                                      coset_gen=g)
            dt = (time.time() - t0) / reps * 1e3
            print(f"2^{log_n} extend: {dt:7.3f} ms  "
                  f"(2^{log_n - EXT_BITS} coefficients in place)  x{reps}")
        gpu.free(d)
    gpu.close()


if __name__ == "__main__":
    main()
