"""Host side of the wide pass (one wavefront per alignment): the planner that
cuts it into sub-launches over the step-indexed state, and the rule for the
pairs the wave schedule does not cover (src/hip/aligner_plan.cpp). Plain C++,
so it is checked where sanitizers work: a stand-alone program
(tests/aligner_wide_plan_check.cpp) built with the address and
undefined-behaviour sanitizers.
"""

import os
import shutil
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def test_wide_pass_planning_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "aligner_wide_plan_check"
    subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", str(REPO / "src"),
         str(REPO / "tests" / "aligner_wide_plan_check.cpp"),
         str(REPO / "src" / "hip" / "aligner_plan.cpp"), "-o", str(exe)],
        check=True, timeout=120)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "aligner wide plan OK" in p.stdout
