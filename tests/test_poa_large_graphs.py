"""--poa-large-graphs outside the GPU: the flag exists and is documented, does
nothing to a CPU run, is forwarded by the wrapper, and the large capacity
class's slab layout holds its static_asserts in a build without HIP. The
pass itself is tested in test_poa_large_graphs_gpu.py."""

import os
import shutil
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
WRAPPER = REPO / "scripts" / "racon_wrapper.py"


def test_flag_is_in_help(racon_cli):
    out = subprocess.run([racon_cli, "-h"], capture_output=True, text=True, check=True).stdout
    assert "--poa-large-graphs" in out
    assert "--aligner-wide-band" in out  # and it displaced nothing


def test_cpu_run_is_identical_with_the_flag(racon_cli, sample):
    base = [racon_cli, "-t", "4", sample["reads"], sample["overlaps"], sample["layout"]]
    plain = subprocess.run(base, capture_output=True, check=True)
    flagged = subprocess.run(base[:1] + ["--poa-large-graphs"] + base[1:], capture_output=True,
                             check=True)
    assert plain.stdout == flagged.stdout and len(plain.stdout) > 1000
    assert b"large-graph" not in flagged.stderr


def test_python_keyword_defaults_off(racon, sample):
    files = (sample["reads"], sample["overlaps"], sample["layout"])
    assert racon.polish(*files, threads=4, poa_large_graphs=True) == \
        racon.polish(*files, threads=4)


def test_wrapper_forwards_the_flag(tmp_path):
    """In the manner of test_tools.test_wrapper_forwards_gpu_flags."""
    fake = tmp_path / "fake_racon.sh"
    fake.write_text("#!/bin/sh\necho \"$@\"\n")
    fake.chmod(0o755)
    for f in ("reads.fa", "ovl.paf", "tgt.fa"):
        (tmp_path / f).write_text("")
    env = dict(os.environ, RACON_BIN=str(fake), RAMPLER_BIN=str(fake))
    files = [str(tmp_path / f) for f in ("reads.fa", "ovl.paf", "tgt.fa")]
    run = lambda extra: subprocess.run(
        [sys.executable, str(WRAPPER), "-c", "2"] + extra + files,
        capture_output=True, text=True, env=env, cwd=tmp_path, check=True).stdout
    assert "--poa-large-graphs" in run(["--poa-large-graphs"])
    assert "--poa-large-graphs" not in run([])


def test_large_layout_static_asserts_compile_without_hip():
    """hip_polisher_stub.cpp is the backend of a build without HIP and
    includes poa_types.hpp: the pinned slab sizes of both capacity classes
    and the large variant's LDS budget are checked by the host compiler."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None
    stub = REPO / "src" / "hip" / "hip_polisher_stub.cpp"
    assert "hip/poa_types.hpp" in stub.read_text()
    header = (REPO / "src" / "hip" / "poa_types.hpp").read_text()
    assert "poa_slab_bytes<true>() == 14384780" in header
    done = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", str(REPO / "src"),
                           str(stub)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
