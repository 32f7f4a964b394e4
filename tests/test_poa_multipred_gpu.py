"""Parity tests for the multi-predecessor DP rows of the HIP POA kernel.

A DP row whose graph node has more than one in-edge takes its maximum over
keys, (score << 6) | (63 - edge), so that the move byte's edge index is the
first edge that attains the maximum, and finds the rows of in-edges 0..4 in
its two row descriptor words; from in-edge 5 on it looks them up in the graph
arrays (src/hip/poa_kernel.hip: dp_row, pred_row_of, build_row_desc). The
windows here put such rows where that code can go wrong: nodes of in-degree
2, 3, 4, 5, 6 and 8 with a later layer through every in-edge, equal
candidates from two in-edges (diagonal, vertical, and diagonal == vertical),
predecessors in the LDS ring and in the global matrix feeding one maximum,
partial layers that cut some or all in-edges of a row, the column-0 chain
through a row whose best edge is not edge 0, row lengths of 1, of a multiple
of 8 and of more than 512 columns, and one window for each kernel
instantiation, banded ones included.

How the shapes are built. At a site p of the backbone, T = backbone[p + 1]
collects in-edges: from backbone[p] (in-edge 0), from a node for each other
letter substituted at p (ring partners of backbone[p], so their branches are
equally long), from backbone[p - k] for a layer that lacks the k bases ending
at p, and from the last node of a run inserted behind p. The sources of the
deletion edges lie k or more ranks in front of T, beyond the four rows of the
LDS ring from k = 4 on; their rows carry the store flag and are read from the
global matrix. Every variant is carried by two layers, so the second runs
through the in-edge the first created. Each test asserts on the graph read
back from the device (rank and out-edges) that its shape is really there.
The tie windows are literal (TIE_WINDOWS): there the edge that wins a tie
decides how many nodes and edges the graph has, and the test asserts both.

Reference: poa_windows_cpu on identical inputs; consensus string and polished
flag must both be equal. Every base carries its own quality, so the
heaviest-bundle walk has no uniform-weight tie (docs/PARITY.md).
"""

import random

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def require_gpu(racon):
    # torch is deliberately not imported here (see test_gpu_kernel_edges.py)
    if racon.device_count() < 1:
        pytest.skip("no GPU on this host")


# --------------------------------------------------------------------------
# input builders (from test_poa_traceback_gpu.py)
# --------------------------------------------------------------------------

def _rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _no_repeat_seq(rng, n):
    """No two neighbours equal: a single-base insertion or deletion has one
    placement only."""
    out = [rng.choice("ACGT")]
    while len(out) < n:
        out.append(rng.choice([c for c in "ACGT" if c != out[-1]]))
    return "".join(out)


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


def _qual(rng, n):
    """Per-base qualities with weights 1..93."""
    return "".join(chr(34 + rng.randrange(93)) for _ in range(n))


def _window(rng, bb, layers):
    blen = len(bb)
    out = [(bb, _qual(rng, blen), 0, 0)]
    for item in layers:
        seq, begin, end = item if isinstance(item, tuple) else (item, 0, blen - 1)
        assert seq, "empty layer"
        out.append((seq, _qual(rng, len(seq)), begin, end))
    return out


# --------------------------------------------------------------------------
# fan sites
# --------------------------------------------------------------------------

def _fan_backbone(rng, blen, sites):
    """A backbone without equal neighbours with fixed bases around every
    site p: backbone[p:p + 2] is "AC", and "A" occurs nowhere in the six
    bases in front, so a deleted block that ends at p cannot be moved to the
    left. Longer deletions can still be placed in more than one way; both
    engines break such ties alike, and what the tests rely on is asserted on
    the graph read back from the device, not assumed."""
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
    """One edit at site p. s0..s2: the other letters at p; d1..d5: the k
    bases ending at p missing; i1, i5: a run of 1 / 5 bases inserted behind
    p; t1: the second other letter at p and backbone[p + 1] missing (the
    vertical move into the row behind T ties between two in-edges)."""
    others = [c for c in "ACGT" if c != bb[p]]
    if kind == "bb":
        return bb
    if kind[0] == "s":
        return bb[:p] + others[int(kind[1])] + bb[p + 1:]
    if kind[0] == "d":
        k = int(kind[1])
        return bb[:p - k + 1] + bb[p + 1:]
    if kind[0] == "i":
        run = {"i1": "G", "i5": "GTGCG"}[kind]  # backbone[p:p + 2] is "AC"
        return bb[:p + 1] + run + bb[p + 1:]
    if kind == "t1":
        return bb[:p] + others[1] + bb[p + 2:]
    raise ValueError(kind)


def _fan_window(rng, blen, sites, kinds, extra=(), plain=2):
    """Every variant at every site twice, plus `plain` copies of the
    backbone and the `extra` layers."""
    bb = _fan_backbone(rng, blen, sites)
    layers = [bb] * plain
    for p in sites:
        for kind in kinds:
            layers += [_variant(bb, p, kind)] * 2
    layers += [e(bb) if callable(e) else e for e in extra]
    return _window(rng, bb, layers)


DEGREE_KINDS = {
    2: ("s0",),
    3: ("s0", "s1"),
    4: ("s0", "s1", "s2"),
    5: ("s0", "s1", "s2", "d1"),
    6: ("s0", "s1", "s2", "d1", "d2"),
    8: ("s0", "s1", "s2", "d1", "d2", "d3", "d4"),
}
DEL_FAN = ("d1", "d2", "d3", "d4", "d5")
SITE = 40


def degree_windows():
    rng = random.Random(11000)
    return [(f"degree {k}", _fan_window(rng, 61 + 9 * k, (SITE,), kinds))
            for k, kinds in DEGREE_KINDS.items()]


# Tie windows: backbone, the edits (begin, end, replacement) that each make
# one layer, carried twice, and the size (nodes, edges) of the graph that the
# CPU engine builds, with the size that the wrong rule would give. They were
# found by a search over small edits at one fan site and checked against a
# copy of the CPU engine's traceback with the tie rule reversed (BASELINE.md,
# "Multi-predecessor DP rows"). In each, two in-edges of one row give the
# same candidate for a cell on the chosen path, and they come from nodes that
# are no ring partners, so the edge that wins decides which nodes and edges
# the layer adds. Sizes do not depend on the qualities.
TIE_WINDOWS = {
    # two in-edges tie for the diagonal candidate; the last one winning
    # gives (65, 66)
    "tie diagonal": ("CACTGCGATAGCTGTGCTACTGCACGATATCTGTGTCTGTACTGCTCGTGAGAGCTGCTAGCTC",
                     ((39, 41, ""), (38, 41, "T")), (64, 66)),
    # two in-edges tie for the vertical candidate; the last one winning
    # gives (73, 78)
    "tie vertical": ("CGATACACTGAGCGCATAGTGATAGAGATGATCGTGCGTGACACACGCGTCTATCACTCGTAGCATCAGC",
                     ((40, 41, "G"), (38, 41, "GGC"), (38, 42, "ATG")), (73, 77)),
    # the diagonal and the vertical candidate are equal (bd == bu) and come
    # through different in-edges; vertical winning gives (73, 76)
    "tie diagonal == vertical": (
        "TGATGCTCTCACGACGCACGATGTATAGCAGTGCGTCTGTACAGTATCTCGTAGTGCGCGTATACGACTA",
        ((38, 41, ""), (37, 41, "GACCC")), (74, 77)),
}


def tie_windows():
    rng = random.Random(11100)
    wins = []
    for tag, (bb, edits, _) in TIE_WINDOWS.items():
        layers = [bb]
        for begin, end, mid in edits:
            layers += [bb[:begin] + mid + bb[end:]] * 2
        wins.append((tag, _window(rng, bb, layers + [bb])))
    return wins


def global_windows():
    """Predecessors at rank distances 1..6 in one row (deletion fan), and a
    run of five inserted bases beside the backbone (distances 1 and 6)."""
    rng = random.Random(11200)
    return [("global deletion fan", _fan_window(rng, 100, (SITE,), DEL_FAN)),
            ("global two fans", _fan_window(rng, 130, (SITE, 90), DEL_FAN + ("s0",))),
            ("global inserted run", _fan_window(rng, 90, (SITE,), ("i5", "i1", "d4")))]


def partial_windows():
    """Layers on a span that begins at p (T's in-edges from the deletions are
    cut, the one from backbone[p] is not) and at p + 1 (every in-edge of the
    span's first row is cut: the virtual start). Exact copies and copies with
    a substitution in the middle; also a one-base layer on T alone."""
    rng = random.Random(11300)
    wins = []
    for blen, end in ((120, 119), (110, 80)):
        bb = _fan_backbone(rng, blen, (SITE,))
        layers = [bb, bb]
        for kind in DEL_FAN + ("s0", "s1"):
            layers += [_variant(bb, SITE, kind)] * 2
        for begin in (SITE, SITE + 1, SITE - 1):
            piece = bb[begin:end + 1]
            mid = len(piece) // 2
            sub = piece[:mid] + next(c for c in "ACGT" if c != piece[mid]) + piece[mid + 1:]
            layers += [(piece, begin, end), (sub, begin, end), (piece, begin, end)]
        wins.append((f"partial end={end}", _window(rng, bb, layers)))
    bb = _fan_backbone(rng, 100, (SITE,))
    layers = [bb, bb]
    for kind in DEL_FAN:
        layers += [_variant(bb, SITE, kind)] * 2
    layers += [(bb[SITE + 1], SITE + 1, SITE + 1), (bb[SITE + 1:SITE + 9], SITE + 1, SITE + 8)] * 2
    wins.append(("partial one base", _window(rng, bb, layers)))
    return wins


def column0_windows():
    """Layers that lack the bases up to behind the fan: the walk reaches
    column 0 below T and climbs through T's row, whose best column-0 edge is
    the longest deletion, not in-edge 0."""
    rng = random.Random(11400)
    wins = []
    for missing in (SITE + 3, SITE + 20):
        wins.append((f"column0 -{missing}",
                     _fan_window(rng, 110, (SITE,), DEL_FAN + ("s0",),
                                 extra=[lambda bb, m=missing: bb[m:]] * 3)))
    return wins


def shape_windows():
    """Row lengths: a multiple of 8 throughout (substitutions only), and
    513..530 columns, which the 8-column variant covers in a second pass."""
    rng = random.Random(11500)
    wins = [(f"shape len={n}", _fan_window(rng, n, (SITE,), ("s0", "s1", "s2")))
            for n in (64, 72, 128)]
    bb = _fan_backbone(rng, 522, (300, 516))
    layers = [bb, bb]
    for n, kind in enumerate(DEL_FAN + ("s0", "s1", "s2")):
        for p in (300, 516):
            v = _variant(bb, p, kind)
            layers += [v, v[:100] + (_no_repeat_seq(rng, n) if n else "") + v[100:]]
    wins.append(("shape two passes", _window(rng, bb, layers)))
    return wins


def variant_windows():
    """One window for each of the narrow, mid and full instantiations; the
    same three shapes serve the banded ones."""
    rng = random.Random(11600)
    kinds = DEL_FAN + ("s0", "s1", "s2")
    return [("variant narrow", _fan_window(rng, 300, (SITE, 250), kinds)),
            ("variant mid", _fan_window(rng, 450, (SITE, 400), kinds)),
            ("variant full", _fan_window(rng, 640, (SITE, 600), kinds))]


def all_cases():
    return (degree_windows() + tie_windows() + global_windows() + partial_windows() +
            column0_windows() + shape_windows() + variant_windows())


# --------------------------------------------------------------------------
# graph read-back
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
    """One CPU run, one GPU run and one graph read-back over every window."""
    cases = all_cases()
    windows = [w for _, w in cases]
    cpu = racon.poa_windows_cpu(windows)
    gpu = racon.poa_windows_gpu(windows)
    graphs = racon.poa_window_graph_gpu(windows)
    return cases, cpu, gpu, [_pred_distances(g) for g in graphs]


@pytest.fixture(scope="module")
def sizes(racon, main_batch):
    """Per window tag: (nodes, edges) of the graph read back from the device.
    The node counts must be the CPU engine's."""
    cases = main_batch[0]
    windows = [w for _, w in cases]
    graphs = racon.poa_window_graph_gpu(windows)
    got = {tag: (len(g[1]), sum(len(row) for row in g[2])) for (tag, _), g in zip(cases, graphs)}
    counts = racon.poa_window_node_counts(windows)
    assert [got[tag][0] for tag, _ in cases] == list(counts)
    return got


def _check(main_batch, prefix):
    cases, cpu, gpu, dists = main_batch
    seen = []
    for (tag, w), c, g, d in zip(cases, cpu, gpu, dists):
        if not tag.startswith(prefix):
            continue
        assert c[1], f"{tag}: the CPU engine did not polish the window"
        assert g[1], f"{tag}: GPU window failed over to the CPU"
        assert g == c, (tag, c[0], g[0])
        seen.append((tag, w, d))
    return seen


@pytest.mark.parametrize("degree", sorted(DEGREE_KINDS))
def test_in_degrees(main_batch, sizes, degree):
    """In-degree 2..5 from the row descriptors, 6 and 8 past them. The second
    copy of every variant runs through the in-edge that the first created and
    adds nothing: the graph is the backbone chain plus one node and two edges
    per substitution and one edge per deletion. A layer threaded through the
    wrong in-edge would add to it."""
    (tag, w, dists), = _check(main_batch, f"degree {degree}")
    assert max(len(d) for d in dists) == degree, (tag, sorted({len(d) for d in dists}))
    kinds = DEGREE_KINDS[degree]
    subs = sum(1 for k in kinds if k[0] == "s")
    blen = len(w[0][0])
    assert sizes[tag] == (blen + subs, blen - 1 + 2 * subs + (len(kinds) - subs)), sizes[tag]


def test_equal_candidates(racon, main_batch, sizes):
    """The first in-edge that attains the maximum wins, and diagonal wins
    over vertical: the graph has the size the CPU engine's rule gives, which
    the reversed rule does not give (TIE_WINDOWS)."""
    seen = _check(main_batch, "tie")
    assert len(seen) == 3
    for tag, _, _ in seen:
        assert sizes[tag] == TIE_WINDOWS[tag][2], (tag, sizes[tag])
    # mismatch == 2 * gap: a mismatch costs what a gap pair costs, so many
    # more cells have diagonal == vertical
    windows = [w for _, w, _ in seen]
    kw = dict(match=3, mismatch=-8, gap=-4)
    assert racon.poa_windows_gpu(windows, **kw) == racon.poa_windows_cpu(windows, **kw)
    got = [len(g[1]) for g in racon.poa_window_graph_gpu(windows, **kw)]
    assert got == racon.poa_window_node_counts(windows, **kw)


def test_ring_and_global_predecessors_in_one_row(main_batch):
    seen = _check(main_batch, "global")
    assert len(seen) == 3
    fan = seen[0][2]
    assert any({1, 3, 4} <= set(d) and max(d) >= 5 for d in fan), sorted(map(tuple, fan))[-3:]
    assert sum(1 for d in seen[1][2] if len(d) >= 5 and max(d) >= 5) >= 2
    assert any(len(d) >= 2 and d[0] == 1 and max(d) >= 6 for d in seen[2][2])


def test_partial_layers(main_batch):
    seen = _check(main_batch, "partial")
    assert len(seen) == 3
    for tag, w, dists in seen:
        # T's row: in-edge 0 from the rank in front, deletion edges from further
        assert any(len(d) >= 4 and d[0] == 1 and max(d) >= 4 for d in dists), tag
        assert {l[2] for l in w[1:]} >= {0, SITE + 1}, tag
    assert min(len(l[0]) for l in seen[2][1]) == 1


def test_column0_chain(main_batch):
    seen = _check(main_batch, "column0")
    assert len(seen) == 2
    for tag, w, dists in seen:
        assert any(len(d) >= 6 and max(d) >= 5 for d in dists), tag
        assert min(len(l[0]) for l in w) < len(w[0][0]) - SITE


def test_row_shapes(main_batch):
    seen = _check(main_batch, "shape")
    assert len(seen) == 4
    for tag, w, dists in seen[:3]:
        assert {len(l[0]) % 8 for l in w} == {0}, tag
        assert max(len(d) for d in dists) == 4, tag
    tag, w, dists = seen[3]
    assert all(513 <= len(l[0]) <= 530 for l in w), sorted(len(l[0]) for l in w)
    assert sum(1 for d in dists if len(d) >= 4) >= 2, tag


VARIANT_LENGTHS = {"variant narrow": (1, 320), "variant mid": (321, 575),
                   "variant full": (576, 1023)}


def test_every_instantiation(racon, main_batch):
    seen = _check(main_batch, "variant")
    assert len(seen) == 3
    for tag, w, dists in seen:
        lo, hi = VARIANT_LENGTHS[tag]
        assert lo <= max(len(l[0]) for l in w) <= hi and len(w) <= 97, tag
        assert sum(1 for d in dists if len(d) >= 7) >= 2, tag
    # banded: the mid and full windows go to the banded mid and banded full
    # instantiations (rows wider than the 256-column band)
    windows = [w for _, w, _ in seen[1:]]
    cpu = racon.poa_windows_cpu(windows)
    gpu = racon.poa_windows_gpu(windows, banded=True)
    assert gpu == cpu
    for g in racon.poa_window_graph_gpu(windows, banded=True):
        assert sum(1 for d in _pred_distances(g) if len(d) >= 7) >= 2


def test_batch_order(racon, main_batch):
    """The same windows in shuffled order give the same results."""
    cases, _, gpu, _ = main_batch
    windows = [w for _, w in cases]
    perm = list(range(len(windows)))
    random.Random(11700).shuffle(perm)
    got = racon.poa_windows_gpu([windows[k] for k in perm])
    assert [cases[k][0] for j, k in enumerate(perm) if got[j] != gpu[k]] == []


RING_COLUMN = 70


def overflow_windows():
    """The fail-over shapes of test_poa_traceback_gpu.py: 2000 nodes against
    the 1535-node cap of the mid variant, an insert-heavy 500-base window of 30 layers (1800+
    nodes), and a column with six symbols (a fifth ring partner). The
    existing tests have no window that reaches the edge cap."""
    rng = random.Random(8700)
    exact = _window(rng, "A" * 400, ["C" * 400, "G" * 400, "T" * 400, "N" * 400])
    rng = random.Random(8701)
    bb = _rand_seq(rng, 500)
    heavy = [(bb, "!" * 500, 0, 0)]
    heavy += [(_mutate(rng, bb, 0.05, 0.10, 0.10), "", 0, 499) for _ in range(30)]
    rng = random.Random(8300)
    bb = _rand_seq(rng, 130)
    layers = []
    for s in [c for c in "ACGT" if c != bb[RING_COLUMN]] + ["N", "R"]:
        layer = bb[:RING_COLUMN] + s + bb[RING_COLUMN + 1:]
        layers += [layer, layer]
    ring = _window(rng, bb, layers)
    return exact, heavy, ring


def test_overflows_still_fail_over(racon, main_batch):
    exact, heavy, ring = overflow_windows()
    counts = racon.poa_window_node_counts([exact, heavy])
    assert counts[0] == 2000 and counts[1] >= 1800, counts
    cases, _, gpu, _ = main_batch
    picks = ("degree 8", "global deletion fan", "partial end=80")
    others = [(w, g) for (tag, w), g in zip(cases, gpu) if tag in picks]
    assert len(others) == 3
    mixed = [others[0][0], exact, others[1][0], ring, heavy, others[2][0]]
    got = racon.poa_windows_gpu(mixed)
    assert got[1][1] is False, "the 2000-node window did not fail over"
    assert got[3][1] is False, "the six-symbol column did not fail over"
    assert got[4][1] is False, f"the insert-heavy window ({counts[1]} nodes) did not fail over"
    assert [got[0], got[2], got[5]] == [g for _, g in others]
