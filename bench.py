#!/usr/bin/env python3
"""Flagship benchmark: Mbp polished per second (whole job), ONT-style
synthetic long reads, C. elegans-class config (BASELINE.json).

One process per GPU. The driver launches N>1 via torch.distributed.run,
which only supplies RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* env vars — the
communication itself is the engine's own PyTorch-free component
(src/hip/comm.cpp): TCP control plane for bootstrap/sizes, RCCL over xGMI
for the polished-contig gather (length-prefixed point-to-point sends, no
padded ring). Each rank polishes a fixed-size shard of the synthetic genome
on its own GPU (weak scaling: per-GPU work constant; at --gpus 8 the node
polishes a full C. elegans-sized 100 Mbp genome per step at 30x coverage).
A step is the whole job: parse, align overlaps, route windows, POA
consensus on the GPU, and gather of the polished contigs to rank 0.

Usage: python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints one JSON result
line; that is all the headline figure needs. --dump-outputs DIR additionally
writes what the last timed step returned (see dump_outputs). --full is the
switch for any secondary measurement (baselines, other configurations); the
benchmark has none today, so it currently runs the same work as a plain run.
"""

import argparse
import json
import os
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent
sys.path.insert(0, str(REPO / "build"))
sys.path.insert(0, str(REPO))

# One process per GPU: restrict HIP to this rank's device before any HIP
# init — ALWAYS, also for single-rank runs, so an N=1 measurement on an
# 8-GPU node does not silently spread its in-process batches over all
# devices and misreport single-GPU throughput.
LOCAL_RANK = int(os.environ.get("LOCAL_RANK", 0))
os.environ.setdefault("HIP_VISIBLE_DEVICES", str(LOCAL_RANK))


def log(msg):
    print(msg, file=sys.stderr, flush=True)


# --dump-outputs budget: 64 MB in all; the float32 consensus array gets
# 15 Mi elements (60 MB), the rest is headroom for lengths and headers.
DUMP_MAX_ELEMS = 15 * 1024 * 1024
DUMP_SEED = 20240229


def dump_outputs(outdir, seqs):
    """Writes the polished contigs a caller of the timed path receives.

    seqs: polished sequences in output order (on a multi-rank run, rank 0's
    gathered per-rank consensus blobs). Files:
      contig_lengths.npy  float64, length of every sequence
      consensus.npy       float32, ASCII codes of the concatenated sequences;
                          beyond DUMP_MAX_ELEMS a fixed seeded sample of
                          positions (ascending) is kept instead
      consensus_index.npy float64, the sampled positions (only when sampled)
    """
    import numpy as np

    outdir = Path(outdir)
    outdir.mkdir(parents=True, exist_ok=True)
    lengths = np.array([len(s) for s in seqs], dtype=np.float64)
    codes = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    index_path = outdir / "consensus_index.npy"
    if codes.size > DUMP_MAX_ELEMS:
        rng = np.random.default_rng(DUMP_SEED)
        # a sample costs 12 bytes: float32 value + float64 position
        n = DUMP_MAX_ELEMS // 3
        idx = np.sort(rng.choice(codes.size, size=n, replace=False))
        codes = codes[idx]
        np.save(index_path, idx.astype(np.float64))
    elif index_path.exists():
        index_path.unlink()
    np.save(outdir / "contig_lengths.npy", lengths)
    np.save(outdir / "consensus.npy", codes.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-mbp", type=float, default=None,
                    help="genome Mbp per GPU shard (default 12.5 = C.elegans/8)")
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--window", type=int, default=500)
    ap.add_argument("--threads", type=int, default=None,
                    help="CPU threads per rank (default: ncpu / (2*world))")
    ap.add_argument("--poa-batches", type=int, default=4)
    ap.add_argument("--aligner-batches", type=int, default=6)
    ap.add_argument("--banded", action="store_true",
                    help="use -b static-band POA (approximation; off by default)")
    ap.add_argument("--cpu", action="store_true", help="force CPU path (debug)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's polished contigs as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run secondary measurements (none exist today)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", 1))
    rank = int(os.environ.get("RANK", 0))
    n_gpus = max(args.gpus, world)
    if args.threads is None:
        args.threads = max(8, (os.cpu_count() or 16) // (2 * world))

    import _racon

    have_gpu = _racon.device_count() > 0 and not args.cpu
    # Honest default: the BASELINE config is 12.5 Mbp/GPU (100 Mbp at 8 GPUs).
    # Without a GPU the CPU path cannot finish that in minutes; shrink and say so.
    genome_mbp = args.genome_mbp if args.genome_mbp is not None else (12.5 if have_gpu else 0.3)
    data_tag = "synthetic" if have_gpu and genome_mbp >= 12.5 else "synthetic-reduced"

    if world > 1:
        # RCCL data plane needs one distinct GPU per rank; a single-GPU
        # rehearsal (two ranks pinned to the same device) sets
        # RGA_COMM_FORCE_TCP=1 to exercise the full multi-process flow with
        # the loopback data plane instead.
        use_rccl = have_gpu and os.environ.get("RGA_COMM_FORCE_TCP", "0") != "1"
        host = os.environ.get("MASTER_ADDR", "127.0.0.1")
        port = int(os.environ.get("RGA_COMM_PORT",
                                  int(os.environ.get("MASTER_PORT", "29476")) + 41))
        _racon.comm_init(rank, world, host, port, use_rccl)

    from racon_amd import synth

    # -------- setup (untimed): per-rank shard of the synthetic genome --------
    shard_bp = int(genome_mbp * 1e6)
    work = Path(os.environ.get("TMPDIR", "/tmp")) / f"racon_bench_r{rank}_{shard_bp}_{args.coverage}"
    marker = work / "done"
    if not marker.exists():
        log(f"[rank {rank}] generating shard: {genome_mbp} Mbp x {args.coverage}x ...")
        synth.make_sample(work, genome_bp=shard_bp, coverage=args.coverage,
                          seed=1234 + rank, read_len_mean=15000, read_len_sd=5000)
        marker.touch()
    sample = {
        "reads": str(work / "reads.fasta"),
        "overlaps": str(work / "overlaps.paf"),
        "layout": str(work / "layout.fasta"),
    }

    poa_batches = args.poa_batches if have_gpu else 0
    aligner_batches = args.aligner_batches if have_gpu else 0

    def one_step():
        out = _racon.polish(sample["reads"], sample["overlaps"], sample["layout"],
                            threads=args.threads, window_length=args.window,
                            poa_batches=poa_batches, aligner_batches=aligner_batches,
                            banded_poa=args.banded)
        # gather polished contigs to rank 0: length-prefixed point-to-point
        # over RCCL/xGMI (comm.cpp) — each rank's exact bytes, no padding
        received = out
        if world > 1:
            blob = "".join(s for _, s in out).encode()
            parts = _racon.comm_gather(blob, 0)
            if rank == 0:
                assert len(parts) == world
            received = parts
        return sum(len(s) for _, s in out), received

    def barrier_sync():
        # barrier + full device sync on both sides of the timed region
        # (equivalent of dist.barrier() + torch.cuda.synchronize())
        if world > 1:
            _racon.comm_barrier()
        if have_gpu:
            _racon.device_synchronize()

    for w in range(args.warmup):
        one_step()
        log(f"[rank {rank}] warmup {w + 1}/{args.warmup} done")

    barrier_sync()
    t0 = time.perf_counter()
    polished_bp = 0
    received = []
    for _ in range(args.steps):
        step_bp, received = one_step()
        polished_bp += step_bp
    barrier_sync()
    elapsed = time.perf_counter() - t0

    # whole-job numbers: MAX time over ranks, SUM of polished bp
    if world > 1:
        elapsed = _racon.comm_allreduce_max(elapsed)
        polished_bp = _racon.comm_allreduce_sum(float(polished_bp))

    if rank == 0 and args.dump_outputs:
        if world > 1:
            seqs = [bytes(p) for p in received]
        else:
            seqs = [s.encode() for _, s in received]
        dump_outputs(args.dump_outputs, seqs)

    if rank == 0:
        value = polished_bp / 1e6 / elapsed
        print(json.dumps({
            "metric": "Mbp polished/sec (whole node), ONT C.elegans, at 1/2/4/8 MI355X",
            "value": round(value, 4),
            "unit": "Mbp/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed * 1000 / args.steps, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "int16",
            "data": data_tag,
            "config": {
                "model": "racon-polish ONT synthetic (C.elegans-class at 8 GPUs)",
                "genome_mbp_per_gpu": genome_mbp,
                "coverage": args.coverage,
                "window_length": args.window,
                "read_len_mean": 15000,
                "error_profile": "2%sub+2%ins+2%del",
                "poa_batches": poa_batches,
                "aligner_batches": aligner_batches,
                "parallelism": f"dp{n_gpus}",
            },
        }))

    if world > 1:
        _racon.comm_finalize()


if __name__ == "__main__":
    main()
