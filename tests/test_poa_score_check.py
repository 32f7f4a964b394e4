"""--poa-score-check outside the GPU: the flag exists and is documented, does
nothing to a CPU run, is forwarded by the wrapper; the rule (poa_types.hpp)
compiles without HIP and is what this file restates; and the CPU model of the
device check (poa_window_score_bounds) is sound: no DP cell lies below what
the check compares with the floor, none above the static bound. The device
side is tested in test_poa_score_check_gpu.py."""

import os
import random
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
WRAPPER = REPO / "scripts" / "racon_wrapper.py"

FLOOR = -28000
WIDTH = 1024  # kPoaLimits.matrix_width, both capacity classes

HEAVY = (0.05, 0.10, 0.10)
ONT = (0.03, 0.03, 0.04)


# the rule, restated (src/hip/poa_types.hpp)
def static_ok(m, x, g):
    return g < 0 and max(m, x, 0) * (WIDTH - 1) <= -FLOOR


def row_refused(h0, length, g):
    return h0 + length * g < FLOOR


def test_flag_is_in_help(racon_cli):
    out = subprocess.run([racon_cli, "-h"], capture_output=True, text=True, check=True).stdout
    assert "--poa-score-check" in out
    assert "--poa-large-graphs" in out  # and it displaced nothing
    # the help says that -b keeps the old guard
    text = " ".join(out[out.index("--poa-score-check"):].split())
    assert "none with -b" in text


def test_cpu_run_is_identical_with_the_flag(racon_cli, sample):
    base = [racon_cli, "-t", "4", sample["reads"], sample["overlaps"], sample["layout"]]
    plain = subprocess.run(base, capture_output=True, check=True)
    flagged = subprocess.run(base[:1] + ["--poa-score-check"] + base[1:], capture_output=True,
                             check=True)
    assert plain.stdout == flagged.stdout and len(plain.stdout) > 1000
    assert b"score check" not in flagged.stderr


def test_python_keywords_default_off(racon, sample):
    files = (sample["reads"], sample["overlaps"], sample["layout"])
    assert racon.polish(*files, threads=4, poa_score_check=True) == \
        racon.polish(*files, threads=4)
    for name in ("polish", "poa_windows_gpu", "poa_window_graph_gpu"):
        doc = getattr(racon, name).__doc__
        assert "score_check: bool = False" in doc, (name, doc)


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
    assert "--poa-score-check" in run(["--poa-score-check"])
    assert "--poa-score-check" not in run([])
    both = run(["--poa-score-check", "--poa-large-graphs"])
    assert "--poa-score-check" in both and "--poa-large-graphs" in both


_RULE_MAIN = """
#include <cstdio>
#include <cstdlib>
#include "hip/poa_types.hpp"
int main(int argc, char** argv) {
  using namespace rga::hip;
  static_assert(kPoaScoreFloor == -28000 && kPoaScoreRange == 7);
  static_assert(kPoaLimits.matrix_width == 1024 && kPoaLargeLimits.matrix_width == 1024);
  for (int i = 1; i + 3 < argc; i += 4) {
    const int a = atoi(argv[i + 1]), b = atoi(argv[i + 2]), c = atoi(argv[i + 3]);
    if (argv[i][0] == 's') {
      printf("%d\\n", poa_score_check_static(a, b, c, kPoaLimits.matrix_width) ? 1 : 0);
    } else {
      printf("%d\\n", poa_score_row_refused(a, static_cast<uint32_t>(b), c) ? 1 : 0);
    }
  }
  return 0;
}
"""


def test_rule_compiles_without_hip_and_matches(tmp_path):
    """poa_types.hpp needs no HIP header: a host program built from it gives
    the rule's answers at the boundary values, and they are the restatement's."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None
    src = tmp_path / "rule.cpp"
    src.write_text(_RULE_MAIN)
    exe = tmp_path / "rule"
    done = subprocess.run([cxx, "-std=c++17", "-I", str(REPO / "src"), str(src), "-o", str(exe)],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    static_cases = [(27, -20, -13), (28, -20, -13), (3, -5, -4), (3, -5, 0), (3, -5, 1),
                    (-1, -5, -4), (-3, 27, -1), (-3, 28, -1), (0, 0, -128), (127, -5, -4),
                    (8, -6, -8), (10, -10, -10), (12, -9, -11)]
    row_cases = [(-14000, 500, -28), (-14001, 500, -28), (-14500, 500, -29),
                 (-14000, 250, -56), (-14250, 250, -57), (-13999, 250, -56),
                 (-28000, 0, -4), (-28001, 0, -4), (-8, 1023, -27), (-379, 1023, -27),
                 (-380, 1023, -27), (0, 1023, -128), (-17000, 1000, -8), (-20001, 1000, -8)]
    args = []
    for c in static_cases:
        args += ["s"] + [str(v) for v in c]
    for c in row_cases:
        args += ["r"] + [str(v) for v in c]
    out = subprocess.run([str(exe)] + args, capture_output=True, text=True, check=True).stdout
    got = [line == "1" for line in out.split()]
    want = [static_ok(*c) for c in static_cases] + [row_refused(*c) for c in row_cases]
    assert got == want, list(zip(static_cases + row_cases, got, want))
    # the boundary, spelled out
    assert static_ok(27, -20, -13) and not static_ok(28, -20, -13)
    assert not row_refused(-14000, 500, -28) and row_refused(-14500, 500, -29)


# --------------------------------------------------------------------------
# soundness of the model
# --------------------------------------------------------------------------

def _rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _mutate(rng, seq, sub, ins, dele):
    out = []
    for ch in seq:
        r = rng.random()
        if r < dele:
            continue
        if r < dele + ins:
            out.append(rng.choice("ACGT"))
        if r < dele + ins + sub:
            out.append(rng.choice([c for c in "ACGT" if c != ch]))
        else:
            out.append(ch)
    return "".join(out)


def _window(bb, layers):
    blen = len(bb)
    out = [(bb, "!" * blen, 0, 0)]
    for seq in layers:
        out.append((seq[:1023], "", 0, blen - 1))
    return out


def _partial_window(rng, blen, depth, err):
    """Half of the layers cover a part of the backbone only: they go through
    the subgraph path of the CPU engine."""
    bb = _rand_seq(rng, blen)
    out = [(bb, "!" * blen, 0, 0)]
    for k in range(depth):
        if k % 2 == 0:
            out.append((_mutate(rng, bb, *err)[:1023], "", 0, blen - 1))
        else:
            b = rng.randrange(0, blen // 2)
            e = rng.randrange(b + blen // 4, blen)
            out.append((_mutate(rng, bb[b:e + 1], *err)[:1023], "", b, e))
    return out


SCORE_SETS = [(3, -5, -4), (8, -6, -8), (5, -4, -8), (10, -10, -10), (27, -20, -13),
              (1, 2, -1), (-2, -3, -30)]


@pytest.fixture(scope="module")
def random_windows():
    rng = random.Random(8700)
    windows = []
    for k in range(36):
        blen = rng.randrange(200, 601)
        depth = rng.randrange(3, 21)
        err = ONT if k % 2 == 0 else HEAVY
        if k % 3 == 2:
            windows.append(_partial_window(rng, blen, depth, err))
        else:
            bb = _rand_seq(rng, blen)
            windows.append(_window(bb, [_mutate(rng, bb, *err) for _ in range(depth)]))
    return windows


@pytest.mark.parametrize("scores", SCORE_SETS, ids=lambda s: "m%d x%d g%d" % s)
def test_model_is_sound(racon, random_windows, scores):
    """check_min <= true_min: a window that passes the check holds no cell
    below the floor. true_max <= longest layer * max(m, x, 0): the static
    part bounds the cells from above."""
    m, x, g = scores
    assert g < 0
    bounds = racon.poa_window_score_bounds(random_windows, m, x, g)
    assert len(bounds) == len(random_windows)
    for w, (check_min, true_min, true_max) in zip(random_windows, bounds):
        len_max = max(len(layer[0]) for layer in w[1:])
        assert check_min <= true_min, (scores, check_min, true_min)
        assert true_max <= len_max * max(m, x, 0), (scores, true_max, len_max)
        assert true_min <= g and true_min < true_max


def test_model_on_a_chain(racon):
    """Substitution-only layers: every node sits at its position's depth, so
    check_min is -2 * L * |g| exactly, and identical layers score L * m."""
    rng = random.Random(8701)
    L = 300
    bb = _rand_seq(rng, L)
    same = _window(bb, [bb] * 3)
    check_min, true_min, true_max = racon.poa_window_score_bounds([same], 3, -5, -7)[0]
    assert (check_min, true_min, true_max) == (-2 * L * 7, -L * 7, L * 3)
    subs = _window(bb, [_mutate(rng, bb, 0.02, 0.0, 0.0) for _ in range(6)])
    assert racon.poa_window_score_bounds([subs], 3, -5, -7)[0][0] == -2 * L * 7
    with pytest.raises(RuntimeError):
        racon.poa_window_score_bounds([same[:2]])
