"""bench.py command-line contract on the CPU path (tiny shard): the result
line, --steps, --dump-outputs and --full."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent


def run_bench(tmp_path, *extra):
    env = dict(os.environ, TMPDIR=str(tmp_path))
    out = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--warmup", "0",
         "--genome-mbp", "0.03", "--coverage", "10", "--cpu", *extra],
        capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """Two identical runs with --dump-outputs, shared by the tests below."""
    tmp = tmp_path_factory.mktemp("bench")
    recs = [run_bench(tmp, "--steps", "2", "--dump-outputs", str(tmp / f"dump{i}"))
            for i in range(2)]
    return tmp, recs


def test_result_line(dumped):
    _, recs = dumped
    rec = recs[0]
    assert rec["steps"] == 2 and rec["warmup"] == 0
    assert rec["unit"] == "Mbp/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "int16"
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region
    polished_mbp = rec["value"] * rec["ms_per_step"] / 1000
    assert polished_mbp == pytest.approx(0.03, rel=0.05)


def test_dump_outputs_reproducible(dumped):
    tmp, _ = dumped
    a, b = tmp / "dump0", tmp / "dump1"
    assert sorted(p.name for p in a.iterdir()) == ["consensus.npy", "contig_lengths.npy"]
    total = 0
    for name in ("consensus.npy", "contig_lengths.npy"):
        x, y = np.load(a / name), np.load(b / name)
        assert x.dtype in (np.float32, np.float64)
        assert np.array_equal(x, y)
        total += (a / name).stat().st_size
    assert total <= 64 * 1024 * 1024
    cons, lens = np.load(a / "consensus.npy"), np.load(a / "contig_lengths.npy")
    assert lens.tolist() == [float(cons.size)]
    assert set(np.unique(cons).tolist()) <= {float(c) for c in b"ACGT"}


def test_dump_samples_large_outputs(tmp_path, monkeypatch):
    """Beyond the element budget a fixed seeded sample is written."""
    # importing bench pins HIP_VISIBLE_DEVICES if unset; keep that out of
    # this process's environment
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", os.environ.get("HIP_VISIBLE_DEVICES", "0"))
    monkeypatch.syspath_prepend(str(REPO))
    import bench

    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 300)
    seqs = [b"ACGT" * 100, b"TTGCA" * 40]
    bench.dump_outputs(tmp_path / "d0", seqs)
    bench.dump_outputs(tmp_path / "d1", seqs)
    idx = np.load(tmp_path / "d0" / "consensus_index.npy")
    cons = np.load(tmp_path / "d0" / "consensus.npy")
    assert cons.dtype == np.float32 and idx.dtype == np.float64
    assert idx.size == cons.size == 100
    assert np.all(np.diff(idx) > 0)
    whole = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    assert np.array_equal(cons, whole[idx.astype(np.int64)].astype(np.float32))
    assert np.array_equal(idx, np.load(tmp_path / "d1" / "consensus_index.npy"))
    assert np.load(tmp_path / "d0" / "contig_lengths.npy").tolist() == [400.0, 200.0]


def test_full_flag_accepted(tmp_path):
    rec = run_bench(tmp_path, "--steps", "1", "--full")
    assert rec["steps"] == 1 and rec["value"] > 0
