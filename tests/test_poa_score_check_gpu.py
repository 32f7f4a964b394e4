"""The per-window score check of the HIP POA engine (PoaBatch,
score_check=True; racon --poa-score-check): the class-wide int16 guard
(nodes + width) * max(|m|,|x|,|g|) <= 28000 is replaced by a static condition
on the parameters plus one compare per DP row on the device, h0 + len * g <
-28000 refusing the window (status 7, kPoaScoreRange).

Oracles. The CPU engine on identical inputs at the same scores
(poa_windows_cpu); the CPU model of the check (poa_window_score_bounds), with
which every test first proves that its windows lie on the side of the rule it
means them to; node counts from poa_window_node_counts at the score set under
test. Error profile of the mutated windows: ONT = 3/3/4 % (sub, ins, del).

Tiers, as in test_poa_large_graphs_gpu.py. T0: byte-equal to the CPU
consensus. T1 (assert_t1 of test_gpu_kernel_edges.py): ed <= max(4, len //
100). The windows of the large-graph pass at medaka's scores (8,-6,-8) and the
reference's (5,-4,-8) are held to T0 where the controls (500 x 30 and 800 x 12
ONT at the same scores, no option, the regular kernels alone) are T0 in the
same run, and to T1 with them otherwise. Windows at scores beyond the
worst-case guard have no controls (the unchecked kernels refuse the scores)
and are held to T1.

Measured on one MI355X, one window per row, edit distance to the CPU
consensus at the same scores ("misses" = rows that are not byte-equal):

    controls, no option, (8,-6,-8) and (5,-4,-8)
      500 x 30 ONT, 1368 / 1399 nodes, mid variant      0 misses
      800 x 12 ONT, 1400 / 1427 nodes, full variant     0 misses
    large-graph pass with the score check, (8,-6,-8) and (5,-4,-8)
      500 x 60 ONT,  1723 / 1760 nodes                  0 misses
      500 x 130 ONT, 2141 / 2208 nodes                  0 misses
      1000 x 30 ONT, 2640 / 2704 nodes                  0 misses
    regular class with the score check, (10,-10,-10), (12,-9,-11), (27,-20,-13)
      250 x 8 narrow, 500 x 12 mid, 800 x 12 full       0 misses in 9
    boundary windows that run (L = 500, 250, 700)       0 misses

So the controls are T0 there and the windows of the pass are held to T0. The
pipeline test completed 4 windows in the pass, re-polished 4 -> 0 on the CPU,
and the check refused none.
"""

import random
import re

import pytest

pytestmark = pytest.mark.gpu

ONT = (0.03, 0.03, 0.04)
REGULAR_CAP = 2047
MID_CAP = 1535
LARGE_CAP = 4095
FLOOR = -28000
SCORE_RANGE = 7  # kPoaScoreRange

MEDAKA = (8, -6, -8)
REFERENCE = (5, -4, -8)


@pytest.fixture(scope="module", autouse=True)
def require_gpu(racon):
    # torch is deliberately not imported here (see test_gpu_kernel_edges.py)
    if racon.device_count() < 1:
        pytest.skip("no GPU on this host")
    # as in test_poa_large_graphs_gpu.py: the pooled arenas of earlier files
    # would not leave room for a large pool, and the pipeline test's would
    # starve the files that come after
    racon.release_batch_pools()
    yield
    racon.release_batch_pools()


# --------------------------------------------------------------------------
# input builders (from test_poa_large_graphs_gpu.py / test_gpu_kernel_edges.py)
# --------------------------------------------------------------------------

def _rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


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
    """Window in differ form; layer spans use the pipeline's inclusive end."""
    blen = len(bb)
    out = [(bb, "!" * blen, 0, 0)]
    for seq in layers:
        out.append((seq[:1023], "", 0, blen - 1))
    return out


def _mutated_window(rng, blen, depth, err):
    bb = _rand_seq(rng, blen)
    return _window(bb, [_mutate(rng, bb, *err) for _ in range(depth)])


def _sub_only_window(rng, blen, depth, rate):
    bb = _rand_seq(rng, blen)
    return _window(bb, [_mutate(rng, bb, rate, 0.0, 0.0) for _ in range(depth)])


def _max_len(w):
    return max(len(layer[0]) for layer in w)


def _variant(w):
    """The unbanded route (poa_route): narrow, mid or full."""
    n = _max_len(w)
    if n <= 320:
        return "narrow"
    if n <= 575:
        return "mid" if len(w) <= 96 else "full"
    return "full"


def _ed(racon, a, b):
    return 0 if a == b else racon.edit_distance(a, b)


def assert_t1(racon, tag, cpu, gpu):
    assert gpu[1], f"{tag}: GPU window failed over to the CPU"
    assert cpu[1], f"{tag}: the CPU engine did not polish the window"
    ed = _ed(racon, cpu[0], gpu[0])
    print(f"{tag}: ed {ed} to the CPU consensus of {len(cpu[0])} bases")
    assert ed <= max(4, len(cpu[0]) // 100), (tag, ed)


# tag -> (seed, backbone, layers, lowest and highest CPU node count)
SHAPES = {
    "500 x 60": (8800, 500, 60, MID_CAP + 1, REGULAR_CAP),
    "500 x 130": (8801, 500, 130, REGULAR_CAP + 1, LARGE_CAP),
    "1000 x 30": (8802, 1000, 30, REGULAR_CAP + 1, LARGE_CAP),
    "ctl 500 x 30": (8803, 500, 30, 0, 1499),
    "ctl 800 x 12": (8804, 800, 12, 0, 1499),
}
LARGE_TAGS = [t for t in SHAPES if not t.startswith("ctl")]
CONTROL_TAGS = [t for t in SHAPES if t.startswith("ctl")]


def build_windows():
    return {tag: _mutated_window(random.Random(seed), blen, depth, ONT)
            for tag, (seed, blen, depth, _, _) in SHAPES.items()}


@pytest.fixture(scope="module")
def windows():
    return build_windows()


@pytest.fixture(scope="module")
def large_runs(racon, windows):
    """Per score set: node counts, model bounds and CPU consensus of every
    window, the device with both options, and the controls with none."""
    tags = list(windows)
    ws = [windows[t] for t in tags]
    runs = {}
    for scores in (MEDAKA, REFERENCE):
        counts = dict(zip(tags, racon.poa_window_node_counts(ws, *scores)))
        bounds = dict(zip(tags, racon.poa_window_score_bounds(ws, *scores)))
        cpu = dict(zip(tags, racon.poa_windows_cpu(ws, *scores)))
        gpu = dict(zip(tags, racon.poa_windows_gpu(ws, *scores, large_graphs=True,
                                                   score_check=True)))
        controls = dict(zip(CONTROL_TAGS, racon.poa_windows_gpu(
            [windows[t] for t in CONTROL_TAGS], *scores)))
        runs[scores] = (counts, bounds, cpu, gpu, controls)
    return runs


# --------------------------------------------------------------------------
# 1. off is unchanged
# --------------------------------------------------------------------------

def test_off_is_unchanged(racon, windows, capfd):
    """Without score_check the large pass refuses g = -8 with its warning and
    the over-cap windows stay unpolished; scores of 10 make the batch throw."""
    tags = ["ctl 500 x 30", "500 x 130", "1000 x 30"]
    ws = [windows[t] for t in tags]
    counts = racon.poa_window_node_counts(ws, *REFERENCE)
    assert counts[0] <= MID_CAP and counts[1] > REGULAR_CAP and counts[2] > REGULAR_CAP, counts
    capfd.readouterr()
    for kw in (dict(), dict(score_check=False)):
        got = racon.poa_windows_gpu(ws, *REFERENCE, large_graphs=True, **kw)
        err = capfd.readouterr().err
        assert [ok for _, ok in got] == [True, False, False], kw
        assert "warning" in err and "large-graph pass" in err, err
    small = [windows["ctl 500 x 30"]]
    for kw in (dict(), dict(score_check=False), dict(score_check=True, banded=True)):
        with pytest.raises(RuntimeError, match="score parameters too large"):
            racon.poa_windows_gpu(small, 10, -10, -10, **kw)
    # where the static part fails the option changes nothing either
    with pytest.raises(RuntimeError, match="score parameters too large"):
        racon.poa_windows_gpu(small, 28, -10, -10, score_check=True)


# --------------------------------------------------------------------------
# 2. medaka's and the reference's scores through the large pass
# --------------------------------------------------------------------------

@pytest.mark.parametrize("scores", [MEDAKA, REFERENCE], ids=["m8 x-6 g-8", "m5 x-4 g-8"])
def test_large_pass_at_gap_8(racon, windows, large_runs, scores):
    counts, bounds, cpu, gpu, controls = large_runs[scores]
    for tag, (_, _, _, lo, hi) in SHAPES.items():
        assert lo <= counts[tag] <= hi, (tag, counts[tag], lo, hi)
        assert bounds[tag][0] >= FLOOR, (tag, bounds[tag])  # the rule lets it run
        print(f"{tag}: {counts[tag]} nodes, model bounds {bounds[tag]}")
    # "500 x 60" overflows the mid variant only: it must be routed there
    assert _variant(windows["500 x 60"]) == "mid"
    for tag in LARGE_TAGS + CONTROL_TAGS:
        assert gpu[tag][1], f"{tag}: not completed on the device"
    eds = {t: _ed(racon, cpu[t][0], gpu[t][0]) for t in gpu}
    ctl_eds = {t: _ed(racon, cpu[t][0], controls[t][0]) for t in CONTROL_TAGS}
    print(f"edit distances to the CPU consensus at {scores}: {eds}; controls alone: {ctl_eds}")
    t0 = all(controls[t][1] and controls[t] == tuple(cpu[t]) for t in CONTROL_TAGS)
    print("tier:", "T0" if t0 else "T1")
    for tag in CONTROL_TAGS:
        # the options leave a window that needs neither of them untouched
        assert gpu[tag] == controls[tag], tag
    for tag in LARGE_TAGS + CONTROL_TAGS:
        if t0:
            assert gpu[tag][0] == cpu[tag][0], (tag, eds[tag])
        else:
            assert_t1(racon, tag, cpu[tag], gpu[tag])


# --------------------------------------------------------------------------
# 3. inert where the guard passes
# --------------------------------------------------------------------------

@pytest.mark.parametrize("scores", [(3, -5, -4), MEDAKA], ids=["m3 x-5 g-4", "m8 x-6 g-8"])
def test_inert_where_the_guard_passes(racon, windows, scores):
    rng = random.Random(8810)
    ws = [windows["ctl 500 x 30"], windows["ctl 800 x 12"],
          _mutated_window(rng, 250, 8, ONT), _mutated_window(rng, 500, 12, ONT),
          _sub_only_window(rng, 320, 6, 0.02), _sub_only_window(rng, 576, 6, 0.02)]
    assert sorted({_variant(w) for w in ws}) == ["full", "mid", "narrow"]
    assert all(b[0] >= FLOOR for b in racon.poa_window_score_bounds(ws, *scores))
    plain = racon.poa_windows_gpu(ws, *scores)
    assert all(ok for _, ok in plain)
    assert racon.poa_windows_gpu(ws, *scores, score_check=True) == plain
    assert racon.poa_windows_gpu(ws, *scores, score_check=True, large_graphs=True) == plain


# --------------------------------------------------------------------------
# 4. scores beyond the guard, regular class
# --------------------------------------------------------------------------

BEYOND = [(10, -10, -10), (12, -9, -11), (27, -20, -13)]


@pytest.fixture(scope="module")
def beyond_windows():
    rng = random.Random(8820)
    ws = {"narrow": _mutated_window(rng, 250, 8, ONT), "mid": _mutated_window(rng, 500, 12, ONT),
          "full": _mutated_window(rng, 800, 12, ONT)}
    for variant, w in ws.items():
        assert _variant(w) == variant, (variant, _max_len(w))
    return ws


@pytest.mark.parametrize("scores", BEYOND, ids=lambda s: "m%d x%d g%d" % s)
def test_scores_beyond_the_guard(racon, beyond_windows, scores):
    tags = list(beyond_windows)
    ws = [beyond_windows[t] for t in tags]
    m, x, g = scores
    assert (REGULAR_CAP + 1024) * max(abs(m), abs(x), abs(g)) > 28000  # the old guard refuses
    with pytest.raises(RuntimeError, match="score parameters too large"):
        racon.poa_windows_gpu(ws, *scores)
    bounds = racon.poa_window_score_bounds(ws, *scores)
    counts = racon.poa_window_node_counts(ws, *scores)
    cpu = racon.poa_windows_cpu(ws, *scores)
    gpu = racon.poa_windows_gpu(ws, *scores, score_check=True)
    for tag, b, n, c, got in zip(tags, bounds, counts, cpu, gpu):
        assert b[0] >= FLOOR and b[1] >= FLOOR and b[2] <= -FLOOR, (tag, b)
        assert n <= MID_CAP, (tag, n)
        assert_t1(racon, f"{tag} at {scores}, model {b}", c, got)


# --------------------------------------------------------------------------
# 5. the boundary, exactly
# --------------------------------------------------------------------------

# (backbone, variant, last gap that runs): 2 * L * |g| == 28000
BOUNDARY = [(500, "mid", -28), (250, "narrow", -56), (700, "full", -20)]


@pytest.mark.parametrize("blen,variant,gap", BOUNDARY, ids=lambda v: str(v))
def test_boundary(racon, blen, variant, gap):
    """Substitution-only layers: every layer is as long as the backbone and
    every node sits at its position's depth, so check_min is -2 * L * |g| on
    both engines: -28000 runs, one more unit of gap is refused."""
    w = _sub_only_window(random.Random(8830 + blen), blen, 6, 0.02)
    assert _variant(w) == variant and _max_len(w) == blen
    assert 2 * blen * -gap == -FLOOR
    for g, refused in ((gap, False), (gap - 1, True)):
        scores = (3, -5, g)
        check_min = racon.poa_window_score_bounds([w], *scores)[0][0]
        assert check_min == 2 * blen * g, (check_min, blen, g)
        assert (check_min < FLOOR) == refused
        status = racon.poa_window_graph_gpu([w], *scores, score_check=True)[0][0]
        got = racon.poa_windows_gpu([w], *scores, score_check=True)[0]
        print(f"L={blen} g={g}: check_min {check_min}, device status {status}")
        assert status == (SCORE_RANGE if refused else 0), (blen, g, status)
        if refused:
            assert got[1] is False
        else:
            assert_t1(racon, f"L={blen} g={g}", racon.poa_windows_cpu([w], *scores)[0], got)


# --------------------------------------------------------------------------
# 6. a refusal does not leak
# --------------------------------------------------------------------------

def test_refusal_does_not_leak(racon, windows):
    """A window far beyond the rule between windows that run, one of them
    through the large pass: the neighbours are what they are alone."""
    scores = (8, -6, -16)
    refused = windows["1000 x 30"]
    rng = random.Random(8840)
    a = _mutated_window(rng, 250, 8, ONT)
    b = windows["500 x 60"]            # outgrows the mid variant: large pass
    c = windows["ctl 800 x 12"]
    bounds = racon.poa_window_score_bounds([a, refused, b, c], *scores)
    assert bounds[1][0] < FLOOR - 2000, bounds[1]
    assert all(bounds[k][0] >= FLOOR for k in (0, 2, 3)), bounds
    assert racon.poa_window_node_counts([b], *scores)[0] > MID_CAP
    kw = dict(large_graphs=True, score_check=True)
    solo = {k: racon.poa_windows_gpu([w], *scores, **kw)[0]
            for k, w in (("a", a), ("b", b), ("c", c))}
    assert all(ok for _, ok in solo.values()), solo
    assert racon.poa_window_graph_gpu([refused], *scores, score_check=True)[0][0] == SCORE_RANGE
    for order in (["a", "R", "b", "c"], ["c", "b", "R", "a"]):
        ws = [dict(a=a, b=b, c=c, R=refused)[k] for k in order]
        got = dict(zip(order, racon.poa_windows_gpu(ws, *scores, **kw)))
        assert got["R"][1] is False
        for k in ("a", "b", "c"):
            assert got[k] == solo[k], (order, k)
        # without the large pass as well
        got = dict(zip(order, racon.poa_windows_gpu(ws, *scores, score_check=True)))
        assert got["R"][1] is False and got["a"] == solo["a"] and got["c"] == solo["c"]


_TIMED_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import _racon
windows = [[tuple(layer) for layer in w] for w in json.load(open(sys.argv[2]))]
print(json.dumps(_racon.poa_windows_gpu(windows, 8, -6, -16, large_graphs=True,
                                        score_check=True)))
"""


def test_timed_checked_instantiations(racon, windows, beyond_windows, tmp_path):
    """RGA_POA_TIMING selects the TIMED twins of the four checked kernels
    (narrow, mid, full, large), which nothing else launches: one window each
    and a refused one, in a fresh process with the variable set, give what
    this process gives without it."""
    import json
    import os
    import subprocess
    import sys

    assert "RGA_POA_TIMING" not in os.environ  # read once per process
    ws = [beyond_windows["narrow"], windows["1000 x 30"], windows["500 x 60"],
          windows["ctl 800 x 12"], beyond_windows["mid"]]
    assert [_variant(w) for w in ws] == ["narrow", "full", "mid", "full", "mid"]
    want = racon.poa_windows_gpu(ws, 8, -6, -16, large_graphs=True, score_check=True)
    assert [ok for _, ok in want] == [True, False, True, True, True]
    args = tmp_path / "windows.json"
    args.write_text(json.dumps(ws))
    child = subprocess.run(
        [sys.executable, "-c", _TIMED_CHILD, os.path.dirname(racon.__file__), str(args)],
        env=dict(os.environ, RGA_POA_TIMING="1"), capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    assert [tuple(r) for r in json.loads(child.stdout)] == want
    assert child.stderr.count("timing (wall ticks") == 2, child.stderr[-2000:]  # both passes


# --------------------------------------------------------------------------
# 7. pipeline
# --------------------------------------------------------------------------

def _count(pattern, text):
    m = re.search(pattern, text)
    return int(m.group(1)) if m else 0


def test_pipeline(racon, tmp_path, fasta_reader, capfd):
    """The deep-w500 configuration of test_poa_large_graphs_gpu.test_pipeline
    at medaka's scores: the large pass refuses them without the check and
    completes windows with it."""
    from racon_amd import synth

    s = synth.make_sample(tmp_path, seed=31, sub=0.03, ins=0.03, dele=0.04, genome_bp=8000,
                          coverage=150)
    files = (s["reads"], s["overlaps"], s["layout"])
    truth = list(fasta_reader(s["reference"]).values())[0]
    kw = dict(threads=8, window_length=500, match=8, mismatch=-6, gap=-8)

    capfd.readouterr()
    off = racon.polish(*files, poa_batches=1, poa_large_graphs=True, **kw)
    err_off = capfd.readouterr().err
    repolished_off = _count(r"(\d+) window\(s\) re-polished on CPU", err_off)
    assert "warning: score parameters too large" in err_off and "large-graph pass" in err_off
    assert _count(r"(\d+) window\(s\) completed by the large-graph pass", err_off) == 0
    assert repolished_off > 0, err_off

    on = racon.polish(*files, poa_batches=1, poa_large_graphs=True, poa_score_check=True, **kw)
    err_on = capfd.readouterr().err
    completed = _count(r"(\d+) window\(s\) completed by the large-graph pass", err_on)
    repolished_on = _count(r"(\d+) window\(s\) re-polished on CPU", err_on)
    refused = _count(r"(\d+) window\(s\) refused by the score check", err_on)
    print(f"re-polished on CPU: {repolished_off} -> {repolished_on}, large-graph pass "
          f"completed {completed}, score check refused {refused}")
    assert "score parameters too large" not in err_on, err_on
    assert completed > 0, err_on
    assert repolished_on < repolished_off, (repolished_off, repolished_on)

    cpu = racon.polish(*files, **kw)
    ed_cpu = racon.edit_distance(cpu[0][1], truth)
    ed_gpu = racon.edit_distance(on[0][1], truth)
    print(f"ed to the truth: cpu {ed_cpu}, gpu with the check {ed_gpu}, "
          f"gpu without {racon.edit_distance(off[0][1], truth)}")
    assert ed_gpu <= ed_cpu + max(20, ed_cpu // 5), (ed_cpu, ed_gpu)
