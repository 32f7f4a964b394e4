"""Completion counts of the aligner's band policies at long-read scale.

The sets are probe_band_clamp.py's (24 pairs each at 20 kbp / 6 %, 100 kbp /
6 % and 100 kbp / 12 % error, same seed), run under diagonal 256, adaptive
256, retry 256 and diagonal 512. Prints, per set and policy, how many pairs
completed, how many of those with the optimal distance (--exact: one unbanded
CPU alignment per pair), and the wall time of the call, which includes arena
construction and copies: for kernel time run it under
`rocprofv3 --kernel-trace --stats` (the calls are made in the order printed,
and the adaptive kernels are the myers_kernel instantiations whose last
template argument is true).
Run on a GPU box: python tools/probe_adaptive_band.py [--exact] [--sets 0,1,2]
"""
import argparse
import random
import sys
import time

sys.path.insert(0, "build")
import _racon  # noqa: E402

from probe_band_clamp import mutate  # noqa: E402

SETS = ((20000, 0.02), (100000, 0.02), (100000, 0.04))
RUNS = (("diagonal", 256), ("adaptive", 256), ("retry", 256), ("diagonal", 512))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exact", action="store_true",
                    help="also count results with the optimal distance")
    ap.add_argument("--sets", default="0,1,2")
    args = ap.parse_args()
    wanted = {int(k) for k in args.sets.split(",")}

    rng = random.Random(1234)
    for k, (read_len, err) in enumerate(SETS):
        pairs = []
        for _ in range(24):  # generated even when skipped: the sets stay the same
            t = "".join(rng.choice("ACGT") for _ in range(read_len))
            pairs.append((mutate(rng, t, err, err, err), t))
        if k not in wanted:
            continue
        optimum = [_racon.edit_distance(q, t) for q, t in pairs] if args.exact else None
        for policy, band in RUNS:
            t0 = time.perf_counter()
            res = _racon.gpu_align(pairs, band_width=band, band_policy=policy)
            wall = time.perf_counter() - t0
            ok = sum(1 for _, _, st in res if st == 0)
            line = (f"BAND read_len={read_len} err={3 * err:.0%} {policy} {band}: "
                    f"completed {ok}/{len(pairs)}")
            if optimum is not None:
                exact = sum(1 for (_, ed, st), opt in zip(res, optimum) if st == 0 and ed == opt)
                line += f", exact {exact}/{ok}"
            print(line + f", call {wall:.3f} s", flush=True)


if __name__ == "__main__":
    main()
