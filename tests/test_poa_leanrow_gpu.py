"""Parity tests for the lean single-predecessor DP row of the HIP POA kernel.

A DP row whose node has exactly one in-edge, from a row still in the LDS
ring, in an unbanded layer of at most 512 columns, is computed by dp_row_lean
on packed int16 pairs in the 8-wide unchecked kernels (mid and full); every
other row goes through dp_row (src/hip/poa_kernel.hip). Rows of both kinds
alternate inside one layer and read each other's ring and matrix rows, so the
windows here put the borders of that rule next to each other: layer lengths on
both sides of every length at which the code changes (the lane boundary, the
last lean length 512, the two-pass lengths, the per-byte move store at 575),
single predecessors at rank distance 1..3 (ring, lean) and 4 (global
matrix, general), multi-predecessor rows between them, rows whose scores go
to the global matrix for a far successor, partial layers with their virtual
start rows, the column-0 chain, non-ACGT node letters, score sets with many
ties and one outside the packed range, and one window per kernel variant.

Two oracles on every window:
  1. poa_windows_cpu on identical inputs: consensus and polished flag equal.
     Every base carries its own quality (docs/PARITY.md).
  2. the same windows with lean_rows=False: status, every node's rank and
     every node's out-edge list from poa_window_graph_gpu identical. A wrong
     move byte that the consensus survives still changes the graph.
On a build without the switch the argument is left out (_run), and the file
checks its own inputs against the CPU engine.

Only windows whose longest layer exceeds 320 bases reach the 8-wide kernels,
so short layers are partial layers of such windows.
"""

import random

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def require_gpu(racon):
    # torch is deliberately not imported here (see test_gpu_kernel_edges.py)
    if racon.device_count() < 1:
        pytest.skip("no GPU on this host")


def _run(fn, windows, lean, **kw):
    """fn with the lean row on or off; without the switch where the build has
    none (pybind11 refuses an unknown keyword with TypeError)."""
    try:
        return fn(windows, lean_rows=lean, **kw)
    except TypeError:
        return fn(windows, **kw)


# --------------------------------------------------------------------------
# input builders (from test_poa_multipred_gpu.py)
# --------------------------------------------------------------------------

def _no_repeat_seq(rng, n):
    out = [rng.choice("ACGT")]
    while len(out) < n:
        out.append(rng.choice([c for c in "ACGT" if c != out[-1]]))
    return "".join(out)


def _qual(rng, n):
    return "".join(chr(34 + rng.randrange(93)) for _ in range(n))


def _window(rng, bb, layers):
    blen = len(bb)
    out = [(bb, _qual(rng, blen), 0, 0)]
    for item in layers:
        seq, begin, end = item if isinstance(item, tuple) else (item, 0, blen - 1)
        assert seq, "empty layer"
        out.append((seq, _qual(rng, len(seq)), begin, end))
    return out


def _fan_backbone(rng, blen, sites):
    for _ in range(1000):
        bb = list(_no_repeat_seq(rng, blen))
        for p in sites:
            bb[p - 6:p + 2] = "GTCTGTAC"[:8] if bb[p - 7] != "G" else "TGCGTGAC"
            if bb[p + 2] == bb[p + 1]:
                bb[p + 2] = "G" if bb[p + 3] != "G" else "T"
        s = "".join(bb)
        if all(a != b for a, b in zip(s, s[1:])):
            return s
    raise AssertionError("no backbone found")


def _variant(bb, p, kind):
    """One edit at site p. s0..s2: the other letters at p; sN: an N at p;
    d1..d5: the k bases ending at p missing."""
    others = [c for c in "ACGT" if c != bb[p]]
    if kind == "sN":
        return bb[:p] + "N" + bb[p + 1:]
    if kind[0] == "s":
        return bb[:p] + others[int(kind[1])] + bb[p + 1:]
    if kind[0] == "d":
        k = int(kind[1])
        return bb[:p - k + 1] + bb[p + 1:]
    raise ValueError(kind)


def _fan_window(rng, blen, sites, kinds, extra=(), plain=2):
    bb = _fan_backbone(rng, blen, sites)
    layers = [bb] * plain
    for p in sites:
        for kind in kinds:
            layers += [_variant(bb, p, kind)] * 2
    layers += [e(bb) if callable(e) else e for e in extra]
    return _window(rng, bb, layers)


def _subs(rng, seq, count):
    """`count` substitutions at distinct positions."""
    out = list(seq)
    for p in rng.sample(range(len(seq)), count):
        out[p] = rng.choice([c for c in "ACGT" if c != out[p]])
    return "".join(out)


def _dels(rng, seq, count):
    drop = set(rng.sample(range(1, len(seq) - 1), count))
    return "".join(c for i, c in enumerate(seq) if i not in drop)


SUBS = ("s0", "s1", "s2")
DEL_FAN = ("d1", "d2", "d3", "d4", "d5")
SITE = 40

# layer lengths at which the row changes its path
LENGTHS_FULL = (321, 504, 505, 511, 512, 513, 575)
LENGTHS_PARTIAL = (1, 7, 8, 9, 63, 64, 65)


def length_windows():
    """One window per long length n: backbone and substitution-only layers of
    exactly n bases, layers with 1..3 bases missing, and, below 575, one with
    a base more. The short lengths are exact pieces of a 400-base backbone,
    aligned to their span, each once as it is and once with a substitution."""
    rng = random.Random(12000)
    wins = []
    for n in LENGTHS_FULL:
        bb = _no_repeat_seq(rng, n)
        layers = [_subs(rng, bb, 4), _subs(rng, bb, 4), bb]
        layers += [_dels(rng, bb, k) for k in (1, 2, 3)]
        if n < 575:
            p = rng.randrange(10, n - 10)
            layers.append(bb[:p] + next(c for c in "ACGT" if c not in bb[p - 1:p + 1]) + bb[p:])
        wins.append((f"length {n}", _window(rng, bb, layers)))
    bb = _no_repeat_seq(rng, 400)
    layers = [bb, _subs(rng, bb, 4), _subs(rng, bb, 4)]
    for k, n in enumerate(LENGTHS_PARTIAL):
        begin = 30 + 40 * k
        piece = bb[begin:begin + n]
        layers.append((piece, begin, begin + n - 1))
        if n >= 7:
            mid = n // 2
            sub = piece[:mid] + next(c for c in "ACGT" if c != piece[mid]) + piece[mid + 1:]
            layers.append((sub, begin, begin + n - 1))
    wins.append(("length partial", _window(rng, bb, layers)))
    return wins


def variant_windows():
    """Mid, full (more than 96 layers at mid length), narrow, and a long
    window whose rows are two passes; the mid and the long one serve the
    banded variants."""
    rng = random.Random(12100)
    kinds = DEL_FAN + SUBS
    bb = _fan_backbone(rng, 330, (SITE, 250))
    deep = [bb, bb]
    for p in (SITE, 250):
        for kind in kinds:
            deep += [_variant(bb, p, kind)] * 6
    return [("variant mid", _fan_window(rng, 450, (SITE, 400), kinds)),
            ("variant full", _window(rng, bb, deep)),
            ("variant narrow", _fan_window(rng, 300, (SITE, 250), kinds)),
            ("variant long", _fan_window(rng, 640, (SITE, 600), kinds))]


def mixing_windows():
    """Three substitutions and an N at one site: the four partners of
    backbone[p] all hang on backbone[p - 1] alone and follow it in the
    topological order, so single-predecessor rows stand at rank distances 1,
    2 and 3 from their predecessor (in the ring: lean rows) and at 4 (in the
    global matrix: a general row; with the three letters alone the read-back
    showed no distance beyond 3, hence the N in both windows, whose own row
    is a general one too). The row of backbone[p - 1] is itself a
    single-predecessor row that must store its scores for the far one.
    backbone[p + 1] collects the in-edges, with the deletion fan's from
    further back."""
    rng = random.Random(12200)
    return [("mixing fan", _fan_window(rng, 450, (SITE, 300), SUBS + ("sN",) + DEL_FAN)),
            ("mixing len 512",
             _fan_window(rng, 512, (SITE, 480), SUBS + ("sN",) + DEL_FAN[:4]))]


def partial_windows():
    """Spans that begin at p, p + 1 and p - 1 and end inside the backbone or
    at its end; the row of the span's first base loses its only in-edge (the
    virtual start, general row), the one behind it has a usable single
    predecessor (lean row). Plus one-base layers."""
    rng = random.Random(12300)
    wins = []
    for blen, end in ((420, 419), (410, 380)):
        bb = _fan_backbone(rng, blen, (SITE,))
        layers = [bb, bb]
        for kind in DEL_FAN + SUBS[:2]:
            layers += [_variant(bb, SITE, kind)] * 2
        for begin in (SITE, SITE + 1, SITE - 1, 200):
            piece = bb[begin:end + 1]
            mid = len(piece) // 2
            sub = piece[:mid] + next(c for c in "ACGT" if c != piece[mid]) + piece[mid + 1:]
            layers += [(piece, begin, end), (sub, begin, end), (piece, begin, end)]
        wins.append((f"partial end={end}", _window(rng, bb, layers)))
    bb = _fan_backbone(rng, 400, (SITE,))
    layers = [bb, bb] + [_variant(bb, SITE, "d2")] * 2
    layers += [(bb[SITE + 1], SITE + 1, SITE + 1), (bb[200], 200, 200),
               (bb[SITE + 1:SITE + 9], SITE + 1, SITE + 8)] * 2
    wins.append(("partial one base", _window(rng, bb, layers)))
    return wins


def nonacgt_windows():
    """An N early (it becomes a node, whose row is a general one between lean
    rows) and an N in the last layers, over lean rows, matching nothing."""
    rng = random.Random(12400)
    bb = _no_repeat_seq(rng, 400)
    early = bb[:120] + "N" + bb[121:]
    late = bb[:250] + "N" + bb[251:]
    layers = [early, early, _subs(rng, bb, 3), bb, _dels(rng, bb, 2), late, late, bb]
    return [("nonacgt", _window(rng, bb, layers))]


def _homopolymer_seq(rng, n):
    out = []
    while len(out) < n:
        out += [rng.choice([c for c in "ACGT" if not out or c != out[-1]])] * rng.randrange(1, 7)
    return "".join(out[:n])


def tie_windows():
    """Homopolymer runs: an insertion or deletion inside a run can be placed
    anywhere in it, so candidates tie along every run."""
    rng = random.Random(12500)
    wins = []
    for k, n in enumerate((400, 512)):
        bb = _homopolymer_seq(rng, n)
        layers = [bb, _subs(rng, bb, 6), _dels(rng, bb, 5), _dels(rng, bb, 9), _subs(rng, bb, 3),
                  _dels(rng, _subs(rng, bb, 4), 4), bb]
        wins.append((f"tie homopolymer {k}", _window(rng, bb, layers)))
    return wins


# the default, two more in range, and a gap of 0, the nearest set that the
# batch accepts and poa_lean_rows_fit (src/hip/poa_types.hpp) refuses
SCORE_SETS = ((3, -5, -4), (5, -4, -8), (3, -8, -4), (3, -5, 0))


def filler_windows(count):
    rng = random.Random(12600)
    wins = []
    for k in range(count):
        n = rng.randrange(330, 500)
        bb = _no_repeat_seq(rng, n)
        layers = [_dels(rng, _subs(rng, bb, rng.randrange(0, 8)), rng.randrange(0, 6))
                  for _ in range(rng.randrange(4, 9))]
        wins.append((f"filler {k}", _window(rng, bb, layers)))
    return wins


def all_cases():
    cases = (length_windows() + variant_windows() + mixing_windows() + partial_windows() +
             nonacgt_windows() + tie_windows())
    cases += filler_windows(48 - len(cases))
    assert len(cases) == 48
    return cases


# --------------------------------------------------------------------------
# shared runs
# --------------------------------------------------------------------------

def _pred_distances(graph):
    """Per node: the rank distances to the sources of its in-edges."""
    status, rank, edges = graph
    assert status == 0, status
    dist = [[] for _ in rank]
    for u, row in enumerate(edges):
        for v in row:
            assert rank[v] > rank[u]
            dist[v].append(rank[v] - rank[u])
    return [sorted(d) for d in dist]


@pytest.fixture(scope="module")
def main_batch(racon):
    """One CPU run and, with the lean row on and off, one GPU run and one
    graph read-back over all 48 windows."""
    cases = all_cases()
    windows = [w for _, w in cases]
    cpu = racon.poa_windows_cpu(windows)
    gpu = {lean: _run(racon.poa_windows_gpu, windows, lean) for lean in (True, False)}
    graphs = {lean: _run(racon.poa_window_graph_gpu, windows, lean) for lean in (True, False)}
    return cases, cpu, gpu, graphs


def _check(main_batch, prefix):
    """Both oracles on the windows whose tag starts with prefix."""
    cases, cpu, gpu, graphs = main_batch
    seen = []
    for k, (tag, w) in enumerate(cases):
        if not tag.startswith(prefix):
            continue
        assert cpu[k][1], f"{tag}: the CPU engine did not polish the window"
        for lean in (True, False):
            assert gpu[lean][k][1], f"{tag}: GPU window failed over to the CPU (lean={lean})"
            assert gpu[lean][k] == cpu[k], (tag, lean, cpu[k][0], gpu[lean][k][0])
        assert graphs[True][k][0] == 0, (tag, graphs[True][k][0])
        assert graphs[True][k] == graphs[False][k], f"{tag}: the graphs differ"
        seen.append((tag, w, graphs[True][k]))
    return seen


def test_layer_lengths(main_batch):
    seen = _check(main_batch, "length")
    assert len(seen) == len(LENGTHS_FULL) + 1
    for (tag, w, _), n in zip(seen, LENGTHS_FULL):
        lens = sorted(len(l[0]) for l in w)
        assert lens.count(n) >= 3 and lens[-1] <= 575 and lens[0] == n - 3, (tag, lens)
    tag, w, _ = seen[-1]
    assert {len(l[0]) for l in w} >= set(LENGTHS_PARTIAL), tag
    assert max(len(l[0]) for l in w) == 400, tag


def test_kernel_variants(racon, main_batch):
    seen = _check(main_batch, "variant")
    assert len(seen) == 4
    depth = {tag: (max(len(l[0]) for l in w), len(w)) for tag, w, _ in seen}
    assert 321 <= depth["variant mid"][0] <= 575 and depth["variant mid"][1] <= 96
    assert 321 <= depth["variant full"][0] <= 575 and depth["variant full"][1] > 96
    assert depth["variant narrow"][0] <= 320
    assert depth["variant long"][0] > 576
    # banded mid and banded full (rows wider than the 256-column band): the
    # lean row is never taken, the switch must change nothing
    windows = [w for tag, w, _ in seen if tag in ("variant mid", "variant long")]
    cpu = racon.poa_windows_cpu(windows)
    for lean in (True, False):
        assert _run(racon.poa_windows_gpu, windows, lean, banded=True) == cpu, lean
    assert (_run(racon.poa_window_graph_gpu, windows, True, banded=True) ==
            _run(racon.poa_window_graph_gpu, windows, False, banded=True))


def test_path_mixing(main_batch):
    seen = _check(main_batch, "mixing")
    assert len(seen) == 2
    for tag, w, graph in seen:
        assert max(len(l[0]) for l in w) <= 512, tag
        dists = _pred_distances(graph)
        single = {d[0] for d in dists if len(d) == 1}
        # 1..3: in the ring; 4: in the global matrix
        assert single >= {1, 2, 3, 4}, (tag, sorted(single))
        assert any(len(d) >= 5 and d[0] == 1 and max(d) >= 5 for d in dists), tag
        # a single-predecessor ring row (lean) with a successor beyond the
        # ring: its scores are read back from the global matrix
        _, rank, edges = graph
        assert any(len(dists[u]) == 1 and dists[u][0] <= 3 and
                   any(rank[v] - rank[u] >= 4 for v in edges[u])
                   for u in range(len(rank))), tag


def test_partial_layers(main_batch):
    seen = _check(main_batch, "partial")
    assert len(seen) == 3
    for tag, w, _ in seen[:2]:
        assert {l[2] for l in w[1:]} >= {0, SITE - 1, SITE, SITE + 1, 200}, tag
    assert min(len(l[0]) for l in seen[2][1]) == 1


def test_non_acgt(main_batch):
    (tag, w, graph), = _check(main_batch, "nonacgt")
    assert sum(l[0].count("N") for l in w) == 4
    assert len(graph[1]) >= 401  # the N of the early layers became a node


def column0_windows():
    """Layers that lack 1, 8 and 30 leading bases, and layers with 2 and 5
    bases in front of the backbone's first, each three times, so that the
    column-0 chain and row 0's insertions run through lean rows."""
    rng = random.Random(12700)
    wins = []
    for k, missing in enumerate((1, 8, 30)):
        bb = _no_repeat_seq(rng, 380 + 10 * k)
        layers = [bb, _subs(rng, bb, 3)] + [bb[missing:]] * 3 + [_subs(rng, bb, 2)]
        wins.append((f"column0 -{missing}", _window(rng, bb, layers)))
    for extra in (2, 5):
        bb = _no_repeat_seq(rng, 400)
        head = _no_repeat_seq(rng, extra)
        layers = [bb, _subs(rng, bb, 3)] + [head + bb] * 3 + [_subs(rng, bb, 2)]
        wins.append((f"column0 +{extra}", _window(rng, bb, layers)))
    return wins


def test_column0(racon):
    """Untrimmed, as tests/test_poa_traceback_gpu.py compares the windows with
    extra leading bases (the known trim difference, docs/NEXT.md)."""
    cases = column0_windows()
    windows = [w for _, w in cases]
    cpu = racon.poa_windows_cpu(windows, trim=False)
    assert all(c[1] for c in cpu)
    for lean in (True, False):
        got = _run(racon.poa_windows_gpu, windows, lean, trim=False)
        assert [t for (t, _), g, c in zip(cases, got, cpu) if g != c] == [], lean
    graphs = _run(racon.poa_window_graph_gpu, windows, True)
    assert all(g[0] == 0 for g in graphs)
    assert graphs == _run(racon.poa_window_graph_gpu, windows, False)


@pytest.mark.parametrize("scores", SCORE_SETS, ids=lambda s: "m%d_x%d_g%d" % s)
def test_ties(racon, main_batch, scores):
    """Node counts are the CPU engine's and the graphs do not depend on the
    switch, under every score set; 3 / -8 / -4 makes a mismatch cost what two
    gaps cost, so diagonal and up-plus-left tie everywhere."""
    cases = main_batch[0]
    windows = [w for tag, w in cases if tag.startswith(("tie", "mixing", "length 512"))]
    assert len(windows) == 5
    kw = dict(match=scores[0], mismatch=scores[1], gap=scores[2])
    cpu = racon.poa_windows_cpu(windows, **kw)
    for lean in (True, False):
        assert _run(racon.poa_windows_gpu, windows, lean, **kw) == cpu, lean
    graphs = _run(racon.poa_window_graph_gpu, windows, True, **kw)
    assert all(g[0] == 0 for g in graphs)
    assert graphs == _run(racon.poa_window_graph_gpu, windows, False, **kw)
    assert [len(g[1]) for g in graphs] == list(racon.poa_window_node_counts(windows, **kw))
    if scores == SCORE_SETS[0]:
        _check(main_batch, "tie")


def test_batch_order(racon, main_batch):
    """The same 48 windows shuffled and rerun in one batch give the same
    results: a ring column left unwritten shows up as order dependence."""
    cases, _, gpu, graphs = main_batch
    windows = [w for _, w in cases]
    perm = list(range(len(windows)))
    random.Random(12800).shuffle(perm)
    shuffled = [windows[k] for k in perm]
    got = _run(racon.poa_windows_gpu, shuffled, True)
    assert [cases[k][0] for j, k in enumerate(perm) if got[j] != gpu[True][k]] == []
    got = _run(racon.poa_window_graph_gpu, shuffled, True)
    assert [cases[k][0] for j, k in enumerate(perm) if got[j] != graphs[True][k]] == []


def test_fillers(main_batch):
    assert len(_check(main_batch, "filler")) >= 20
