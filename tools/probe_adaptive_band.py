"""Completion counts of the aligner's band policies at long-read scale.

The sets are probe_band_clamp.py's (24 pairs each at 20 kbp / 6 %, 100 kbp /
6 % and 100 kbp / 12 % error, same seed), run under diagonal 256, adaptive
256, retry 256, diagonal 512 and wide (one wavefront per pair, band 4096;
--policies selects, e.g. for one profiler run per policy). Prints, per set and policy, how many pairs
completed, how many of those with the optimal distance (--exact: one unbanded
CPU alignment per pair), and the wall time of the call, which includes arena
construction and copies: for kernel time run it under
`rocprofv3 --kernel-trace --stats` (the calls are made in the order printed,
and the adaptive kernels are the myers_kernel instantiations whose last
template argument is true; the wide band's is myers_wave_kernel).

--sv adds the structural-variant set: 24 pairs of 100 kbp at 6 % with one
block of 300-1500 bases each, query-only in the even pairs and target-only in
the odd ones, run under retry 256, diagonal 512 and retry 256 followed by the
wide pass, and then the CPU aligner's wall time over the pairs retry 256
leaves escaped: what the pipeline would have paid without the wide pass.
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
RUNS = (("diagonal", 256), ("adaptive", 256), ("retry", 256), ("diagonal", 512), ("wide", 0))


def report(tag, res, optimum, wall):
    ok = sum(1 for _, _, st in res if st == 0)
    line = f"{tag}: completed {ok}/{len(res)}"
    if optimum is not None:
        exact = sum(1 for (_, ed, st), opt in zip(res, optimum) if st == 0 and ed == opt)
        line += f", exact {exact}/{ok}"
    print(line + f", call {wall:.3f} s", flush=True)


def sv_set(exact):
    rng = random.Random(4321)
    pairs = []
    for k in range(24):
        t = "".join(rng.choice("ACGT") for _ in range(100000))
        q = mutate(rng, t, 0.02, 0.02, 0.02)
        size = rng.randint(300, 1500)
        at = rng.randint(10000, len(q) - 10000)
        if k % 2 == 0:
            q = q[:at] + "".join(rng.choice("ACGT") for _ in range(size)) + q[at:]
        else:
            q = q[:at] + q[at + size:]
        pairs.append((q, t))
    optimum = [_racon.edit_distance(q, t) for q, t in pairs] if exact else None
    runs = (("retry", 256, False), ("diagonal", 512, False), ("retry", 256, True))
    escaped = []
    for policy, band, wide_pass in runs:
        t0 = time.perf_counter()
        res = _racon.gpu_align(pairs, band_width=band, band_policy=policy, wide_pass=wide_pass)
        wall = time.perf_counter() - t0
        report(f"SV 100 kbp 6% one 300-1500 block {policy} {band}"
               + (" + wide pass" if wide_pass else ""), res, optimum, wall)
        if (policy, wide_pass) == ("retry", False):
            escaped = [p for p, (_, _, st) in zip(pairs, res) if st != 0]
    t0 = time.perf_counter()
    for q, t in escaped:
        _racon.align_cigar(q, t)
    print(f"SV CPU aligner over the {len(escaped)} pairs retry 256 leaves escaped: "
          f"{time.perf_counter() - t0:.3f} s (one thread)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exact", action="store_true",
                    help="also count results with the optimal distance")
    ap.add_argument("--sets", default="0,1,2", help="comma-separated; empty for none")
    ap.add_argument("--policies", default=",".join(sorted({p for p, _ in RUNS})))
    ap.add_argument("--sv", action="store_true", help="also run the structural-variant set")
    args = ap.parse_args()
    wanted = {int(k) for k in args.sets.split(",") if k}
    policies = set(args.policies.split(","))

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
            if policy not in policies:
                continue
            t0 = time.perf_counter()
            res = _racon.gpu_align(pairs, band_width=band, band_policy=policy)
            wall = time.perf_counter() - t0
            report(f"BAND read_len={read_len} err={3 * err:.0%} {policy} {band}", res, optimum,
                   wall)
    if args.sv:
        sv_set(args.exact)


if __name__ == "__main__":
    main()
