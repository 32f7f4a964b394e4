"""The large-graph pass of the HIP POA engine (PoaBatch, large_graphs=True;
racon --poa-large-graphs): windows that end with kPoaNodeOverflow in the
regular slabs (2047 nodes, 1535 in the mid variant) run again in slabs of
4095 nodes before the CPU engine takes what is left.

Oracle: the CPU engine on identical inputs (poa_windows_cpu), full-span
layers, every node count recomputed with poa_window_node_counts and asserted
before a window is trusted. Error profiles (sub, ins, del): HEAVY = 5/10/10 %,
ONT = 3/3/4 %.

Tiers. A completed window equals the CPU consensus byte for byte (T0) where
control windows do: same generator and error profile, fewer layers, CPU count
under 1500, no option, so the regular kernels alone. Where they do not,
controls and large windows alike are held to T1, assert_t1 of
test_gpu_kernel_edges.py: ed <= max(4, len // 100). Measured on one MI355X,
40 windows per row unless noted, "misses" = windows whose consensus differs
from the CPU engine's, with their edit distances:

    regular path, no option (the kernels as they were before the pass)
      500 x 14 HEAVY, 1363-1469 nodes, mid variant     0 misses
      400 x 20 HEAVY, 1275-1381 nodes, mid variant     1 miss   (1)
      600 x 11 HEAVY, 1471-1591 nodes, full variant    1 miss   (1)
      600 x 18 HEAVY, 1840-1951 nodes, full variant    1 miss   (2)
      500 x 30 ONT,   1281-1366 nodes, mid variant     0 misses
      800 x 12 ONT,   1385-1517 nodes, full variant    0 misses
    large-graph pass
      500 x 30 HEAVY,  1885-2000 nodes                 1 miss   (1)
      400 x 100 HEAVY, 2112-2234 nodes, 20 windows     7 misses (1 1 1 1 4 2 1)
      1000 x 30 HEAVY, 3808-3972 nodes, 20 windows     1 miss   (3)
      1000 x 30 ONT,   2597-2718 nodes, 20 windows     0 misses
      500 x 100 ONT,   2063-2169 nodes, 20 windows     0 misses

The engines order the graph differently (Kahn FIFO on the device, a
depth-first order on the CPU), so equal-score alignments can be broken
differently; at 5/10/10 % the regular path already does that now and then.
So: ONT windows are held to T0, HEAVY windows to T1, controls included.
test_controls reruns the second row of the table as its record.
"""

import json
import os
import random
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HEAVY = (0.05, 0.10, 0.10)
ONT = (0.03, 0.03, 0.04)
REGULAR_CAP = 2047
MID_CAP = 1535
LARGE_CAP = 4095


@pytest.fixture(scope="module", autouse=True)
def require_gpu(racon):
    # torch is deliberately not imported here (see test_gpu_kernel_edges.py)
    if racon.device_count() < 1:
        pytest.skip("no GPU on this host")
    # polish() keeps its batch arenas pooled for the life of the process, each
    # sized from the memory that was free when it was built: what earlier
    # test files left would not hold a large pool, and what the pipeline
    # test here leaves would starve the files that come after
    racon.release_batch_pools()
    yield
    racon.release_batch_pools()


# --------------------------------------------------------------------------
# input builders (from test_gpu_kernel_edges.py)
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


def node_overflow_windows():
    """The two shapes of test_gpu_kernel_edges.node_overflow_windows, same
    seed: [0] 1000 bp x 30 HEAVY, near the large cap; [1] 500 bp x 30 HEAVY,
    between the mid variant's cap and the regular one."""
    rng = random.Random(6700)
    big = _mutated_window(rng, 1000, 30, HEAVY)
    small = _mutated_window(rng, 500, 30, HEAVY)
    return [big, small]


# tag -> (backbone, layers, error profile, lowest and highest CPU node count
# the window is built for)
SHAPES = {
    "mid a": (500, 30, HEAVY, MID_CAP + 1, REGULAR_CAP),
    "mid b": (500, 30, HEAVY, MID_CAP + 1, REGULAR_CAP),
    "2048 a": (400, 100, HEAVY, REGULAR_CAP + 1, 2300),
    "2048 b": (400, 100, HEAVY, REGULAR_CAP + 1, 2300),
    "cap wide": (1000, 30, HEAVY, 3500, LARGE_CAP),
    "cap deep": (800, 200, ONT, 3500, LARGE_CAP),
    "over": (1000, 60, HEAVY, LARGE_CAP + 1, 1 << 16),
    "ctl mid heavy": (500, 12, HEAVY, 0, 1499),
    "ctl mid heavy b": (400, 20, HEAVY, 0, 1499),
    "ctl mid ont": (500, 30, ONT, 0, 1499),
    "ctl full ont": (800, 12, ONT, 0, 1499),
    "ctl full ont b": (1000, 6, ONT, 0, 1499),
    "2048 ont": (500, 100, ONT, REGULAR_CAP + 1, 2300),
}
LARGE_TAGS = [t for t in SHAPES if not t.startswith("ctl") and t != "over"]
CONTROL_TAGS = [t for t in SHAPES if t.startswith("ctl")]


def build_windows():
    rng = random.Random(7700)
    return {tag: _mutated_window(rng, blen, depth, err)
            for tag, (blen, depth, err, _, _) in SHAPES.items()}


def assert_tier(racon, tag, cpu, gpu, err=None):
    """T0 for ONT windows, T1 for HEAVY ones (module docstring)."""
    assert gpu[1], f"{tag}: GPU window failed over to the CPU"
    assert cpu[1], f"{tag}: the CPU engine did not polish the window"
    ed = 0 if gpu[0] == cpu[0] else racon.edit_distance(cpu[0], gpu[0])
    print(f"{tag}: ed {ed} to the CPU consensus of {len(cpu[0])} bases")
    if (err or SHAPES[tag][2]) == ONT:
        assert gpu[0] == cpu[0], (tag, ed, len(cpu[0]), len(gpu[0]))
    else:
        assert ed <= max(4, len(cpu[0]) // 100), (tag, ed)


@pytest.fixture(scope="module")
def batch(racon):
    """Every window once through the CPU engine (consensus and node count),
    once through the device with the pass and, the controls, once without."""
    windows = build_windows()
    tags = list(windows)
    ws = [windows[t] for t in tags]
    counts = dict(zip(tags, racon.poa_window_node_counts(ws)))
    for tag, (_, _, _, lo, hi) in SHAPES.items():
        assert lo <= counts[tag] <= hi, (tag, counts[tag], lo, hi)
    # the mid windows are routed to the mid variant: cap 1535, not 2047
    for tag in ("mid a", "mid b"):
        assert len(windows[tag]) <= 96 and max(len(l[0]) for l in windows[tag]) <= 575
    cpu = dict(zip(tags, racon.poa_windows_cpu(ws)))
    gpu = dict(zip(tags, racon.poa_windows_gpu(ws, large_graphs=True)))
    controls = dict(zip(CONTROL_TAGS,
                        racon.poa_windows_gpu([windows[t] for t in CONTROL_TAGS])))
    return windows, counts, cpu, gpu, controls


def test_off_is_unchanged(racon):
    """Without the option, and with large_graphs=False, the two node-overflow
    shapes fail over as they always did; the keyword exists."""
    over = node_overflow_windows()
    counts = racon.poa_window_node_counts(over)
    assert counts[0] >= 2300 and 1800 <= counts[1] < REGULAR_CAP, counts
    assert [ok for _, ok in racon.poa_windows_gpu(over)] == [False, False]
    assert [ok for _, ok in racon.poa_windows_gpu(over, large_graphs=False)] == [False, False]
    racon.poa_windows_gpu(over, large_graphs=True)  # no TypeError


def test_controls(racon, batch):
    """Windows under 1500 nodes, no option: what the tier is measured on."""
    _, _, cpu, gpu, controls = batch
    for tag in CONTROL_TAGS:
        assert_tier(racon, tag, cpu[tag], controls[tag])
        # and the option does not touch a window that needs no second pass
        assert gpu[tag] == controls[tag], tag
    # the record behind the HEAVY tier: 40 controls of one shape
    rng = random.Random(2)
    ws = [_mutated_window(rng, 400, 20, HEAVY) for _ in range(40)]
    assert max(racon.poa_window_node_counts(ws)) < 1500
    for k, (c, g) in enumerate(zip(racon.poa_windows_cpu(ws), racon.poa_windows_gpu(ws))):
        assert_tier(racon, f"ctl 400x20 HEAVY #{k}", c, g, HEAVY)


def test_across_2048(racon, batch):
    """Windows over the mid variant's cap and windows whose node ids need the
    twelfth bit of the adjacency word complete in the large slabs."""
    _, counts, cpu, gpu, _ = batch
    assert all(MID_CAP < counts[t] <= REGULAR_CAP for t in ("mid a", "mid b")), counts
    assert all(REGULAR_CAP < counts[t] <= 2300 for t in ("2048 a", "2048 b")), counts
    assert REGULAR_CAP < counts["2048 ont"] <= 2300, counts
    for tag in ("mid a", "mid b", "2048 a", "2048 b", "2048 ont"):
        assert_tier(racon, tag, cpu[tag], gpu[tag])


def test_near_the_cap(racon, batch):
    _, counts, cpu, gpu, _ = batch
    for tag in ("cap wide", "cap deep"):
        assert 3500 <= counts[tag] <= LARGE_CAP, (tag, counts[tag])
        assert_tier(racon, tag, cpu[tag], gpu[tag])


def test_over_the_cap(racon, batch):
    """A graph beyond 4095 nodes fails over with the option on as well, and
    the windows of the same call are what they are without it."""
    windows, counts, cpu, gpu, controls = batch
    assert counts["over"] > LARGE_CAP, counts["over"]
    assert gpu["over"][1] is False
    for tag in LARGE_TAGS:
        assert gpu[tag][1], tag
    for tag in CONTROL_TAGS:
        assert gpu[tag] == controls[tag], tag
    # next to one other window only
    pair = racon.poa_windows_gpu([windows["over"], windows["2048 a"]], large_graphs=True)
    assert pair[0][1] is False and pair[1] == gpu["2048 a"]


def kahn_fifo(edges):
    """The reference order (test_poa_topo_gpu.py): sources by ascending id,
    then FIFO, every node's out-edges in list order."""
    indeg = [0] * len(edges)
    for row in edges:
        for v in row:
            indeg[v] += 1
    order = [i for i, d in enumerate(indeg) if d == 0]
    head = 0
    while head < len(order):
        for v in edges[order[head]]:
            indeg[v] -= 1
            if indeg[v] == 0:
                order.append(v)
        head += 1
    return order


def test_graph_readback(racon, batch):
    """The graph a window leaves in its large slab: the CPU engine's node
    count, and rank is exactly the Kahn FIFO order of the read-back adjacency
    (node ids from 2048 on go through the widened adjacency word).

    The node count equals the CPU engine's only if every layer was aligned as
    the CPU engine aligns it, so it is asserted on the ONT windows, whose
    profile is T0 (module docstring): one of 2048-2300 nodes, one near the
    cap. The two HEAVY windows are held to everything else; their graphs may
    differ from the CPU engine's by a few nodes where a tie is broken
    differently (measured here: "2048 a" 2193 nodes against 2190)."""
    windows, counts, _, _, _ = batch
    tags = ["2048 ont", "cap deep", "2048 a", "cap wide"]
    assert REGULAR_CAP < counts["2048 ont"] <= 2300 and 3500 <= counts["cap deep"] <= LARGE_CAP
    graphs = racon.poa_window_graph_gpu([windows[t] for t in tags], large_graphs=True)
    for tag, (status, rank, edges) in zip(tags, graphs):
        assert status == 0, (tag, status)
        print(f"{tag}: {len(rank)} nodes on the device, {counts[tag]} on the CPU")
        assert len(rank) == len(edges)
        if SHAPES[tag][2] == ONT:
            assert len(rank) == counts[tag], (tag, len(rank), counts[tag])
        assert len(rank) > REGULAR_CAP + 1
        order = kahn_fifo(edges)
        assert len(order) == len(rank), f"{tag}: the read-back graph has a cycle"
        bad = [r for r, node in enumerate(order) if rank[node] != r]
        assert bad == [], (tag, bad[:8])
    # without the option the same call reports the overflow and no graph
    status, rank, edges = racon.poa_window_graph_gpu([windows["2048 a"]])[0]
    assert status == 1 and rank == [] and edges == []


_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import _racon
windows = [[tuple(layer) for layer in w] for w in json.load(open(sys.argv[2]))]
print(json.dumps(_racon.poa_windows_gpu(windows, large_graphs=True)))
"""


def test_sub_launches(racon, batch, tmp_path):
    """Five overflow windows through a pool of two large slabs (three
    sub-launches, slabs reused) equal the run with the default pool."""
    windows, _, _, gpu, _ = batch
    tags = ["2048 a", "cap deep", "mid a", "cap wide", "2048 b"]
    assert "RGA_POA_LARGE_SLABS" not in os.environ
    args = tmp_path / "windows.json"
    args.write_text(json.dumps([windows[t] for t in tags]))
    child = subprocess.run(
        [sys.executable, "-c", _CHILD, os.path.dirname(racon.__file__), str(args)],
        env=dict(os.environ, RGA_POA_LARGE_SLABS="2"), capture_output=True, text=True,
        timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    got = [tuple(r) for r in json.loads(child.stdout)]
    assert got == [gpu[t] for t in tags]
    assert all(ok for _, ok in got)


def test_composition(racon, batch):
    """Overflow windows interleaved with regular ones: the regular windows
    are what a run of them alone without the option gives, and the overflow
    windows do not depend on their order."""
    windows, _, _, gpu, controls = batch
    order = ["ctl mid heavy", "cap wide", "ctl full ont", "mid a", "2048 a", "ctl mid ont",
             "over", "cap deep", "ctl full ont b", "2048 b", "mid b", "ctl mid heavy b",
             "2048 ont"]
    assert sorted(order) == sorted(SHAPES)
    got = dict(zip(order, racon.poa_windows_gpu([windows[t] for t in order],
                                                large_graphs=True)))
    for tag in CONTROL_TAGS:
        assert got[tag] == controls[tag], tag
    for tag in LARGE_TAGS + ["over"]:
        assert got[tag] == gpu[tag], tag
    rev = [t for t in reversed(order) if t in LARGE_TAGS]
    got = dict(zip(rev, racon.poa_windows_gpu([windows[t] for t in rev], large_graphs=True)))
    assert got == {t: gpu[t] for t in rev}


def test_score_guard(racon, batch, capfd):
    """m5 x-4 g-8 passes the regular class's int16 guard and fails the large
    one's ((4095 + 1024) * 8 > 28000): one warning, no second pass, the
    regular windows as without the option."""
    windows, _, _, _, _ = batch
    tags = ["ctl mid heavy", "cap wide", "ctl full ont", "2048 a"]
    ws = [windows[t] for t in tags]
    counts = racon.poa_window_node_counts(ws, 5, -4, -8)
    assert counts[1] > REGULAR_CAP and counts[3] > REGULAR_CAP, counts
    assert counts[0] <= MID_CAP and counts[2] <= REGULAR_CAP, counts
    off = racon.poa_windows_gpu(ws, 5, -4, -8)
    capfd.readouterr()
    on = racon.poa_windows_gpu(ws, 5, -4, -8, large_graphs=True)
    err = capfd.readouterr().err
    assert on == off
    assert [ok for _, ok in on] == [True, False, True, False]
    lines = [l for l in err.splitlines() if "large-graph pass" in l]
    assert len(lines) == 1 and "warning" in lines[0], err


def test_banded(racon):
    """1000 bp overflow windows with banded rows in the large variant, held to
    the bound of test_poa_banded_boundaries (ed <= 2 to the CPU engine): one
    at the ONT profile and one at that test's own 2/2/2 %, at which 1000 bp x
    30 layers overflows as well. The large variant is the only
    8-columns-per-lane kernel that runs banded rows, and the last column of a
    band needs a store of its own there (dp_row, tail_col); without it these
    windows came back ok with edit distances of 106 and 130."""
    for seed, err in ((7800, ONT), (7801, (0.02, 0.02, 0.02))):
        w = _mutated_window(random.Random(seed), 1000, 30, err)
        assert max(len(layer[0]) for layer in w) > 576  # wider than the band's 320 columns
        count = racon.poa_window_node_counts([w])[0]
        assert REGULAR_CAP < count <= LARGE_CAP, count
        assert racon.poa_windows_gpu([w], banded=True)[0][1] is False
        cpu = racon.poa_windows_cpu([w])[0]
        gpu = racon.poa_windows_gpu([w], banded=True, large_graphs=True)[0]
        assert gpu[1], "the banded window did not complete in the large slabs"
        ed = racon.edit_distance(cpu[0], gpu[0])
        print(f"banded 1000 bp, {count} nodes: ed {ed}")
        assert ed <= 2, ed


def _count(pattern, text):
    m = re.search(pattern, text)
    return int(m.group(1)) if m else 0


@pytest.mark.parametrize("config", [
    dict(genome_bp=8000, coverage=150),
    dict(genome_bp=8000, coverage=40, window_length=1000),
], ids=["deep-w500", "w1000"])
def test_pipeline(racon, tmp_path, fasta_reader, capfd, config):
    """End to end at ONT-like error: windows that were polished twice, on the
    GPU and then again on the CPU, complete on the GPU with the option."""
    from racon_amd import synth

    config = dict(config)
    window_length = config.pop("window_length", 500)
    s = synth.make_sample(tmp_path, seed=31, sub=0.03, ins=0.03, dele=0.04, **config)
    files = (s["reads"], s["overlaps"], s["layout"])
    truth = list(fasta_reader(s["reference"]).values())[0]
    kw = dict(threads=8, window_length=window_length)

    capfd.readouterr()
    off = racon.polish(*files, poa_batches=1, **kw)
    err_off = capfd.readouterr().err
    repolished_off = _count(r"(\d+) window\(s\) re-polished on CPU", err_off)
    assert repolished_off > 0, err_off
    assert "large-graph pass" not in err_off

    on = racon.polish(*files, poa_batches=1, poa_large_graphs=True, **kw)
    err_on = capfd.readouterr().err
    completed = _count(r"(\d+) window\(s\) completed by the large-graph pass", err_on)
    repolished_on = _count(r"(\d+) window\(s\) re-polished on CPU", err_on)
    print(f"re-polished on CPU: {repolished_off} -> {repolished_on}, "
          f"large-graph pass completed {completed}")
    assert completed > 0, err_on
    assert repolished_off - repolished_on >= completed, (repolished_off, repolished_on, completed)

    cpu = racon.polish(*files, **kw)
    ed_cpu = racon.edit_distance(cpu[0][1], truth)
    ed_gpu = racon.edit_distance(on[0][1], truth)
    print(f"ed to the truth: cpu {ed_cpu}, gpu with the pass {ed_gpu}, "
          f"gpu without {racon.edit_distance(off[0][1], truth)}")
    assert ed_gpu <= ed_cpu + max(20, ed_cpu // 5), (ed_cpu, ed_gpu)

    two = racon.polish(*files, poa_batches=2, poa_large_graphs=True, **kw)
    assert two == on
