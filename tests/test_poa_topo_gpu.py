"""Order tests for topo_sort_d of the HIP POA kernel.

The kernel's topological order is the Kahn FIFO order: sources by ascending
node id, then every popped node's out-edges in list order. topo_sort_d runs
that FIFO from LDS (src/hip/poa_kernel.hip: in-degrees, queue and one packed
word of out-adjacency per node are staged 64 nodes at a time, the queue is
seeded with a ballot/popcount prefix, a node with two or more out-edges reads
the rest of its edge row eight edges per load). The order itself is checked
here, not only what follows from it: _racon.poa_window_graph_gpu reads back
rank and the out-adjacency from the window's slab, the FIFO is recomputed in
Python, and rank[order[r]] == r must hold for every r.

Shapes: node counts around the 64-node staging blocks, sources in different
blocks, out-degrees 0, 1, 2, exactly 8 (one full load) and 10 (a second
load), one window per LDS ring variant, and the batch reversed and shuffled.
Consensus reference: poa_windows_cpu on identical inputs, every base with its
own quality (docs/PARITY.md). Every window must be polished on the device.

Windows are 64-600 bases with 3-16 layers, with one exception the node counts
force: a graph of 63 nodes cannot grow from a backbone of 64 bases, so that
window has 61.
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
# input builders (from test_poa_add_alignment_gpu.py)
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


def _qual(rng, n):
    """Per-base qualities with weights 1..93."""
    return "".join(chr(34 + rng.randrange(93)) for _ in range(n))


def _window(rng, bb, layers):
    """Window in differ form; a layer is a sequence spanning the backbone or
    (sequence, begin, end) with the pipeline's inclusive end."""
    blen = len(bb)
    out = [(bb, _qual(rng, blen), 0, 0)]
    for item in layers:
        seq, begin, end = item if isinstance(item, tuple) else (item, 0, blen - 1)
        assert seq, "empty layer"
        out.append((seq, _qual(rng, len(seq)), begin, end))
    assert 3 <= len(out) - 1 <= 16
    return out


def _sub_at(seq, pos, shift=1):
    """seq with the base at pos replaced by the shift-th next letter."""
    return seq[:pos] + "ACGT"[("ACGT".index(seq[pos]) + shift) % 4] + seq[pos + 1:]


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------

# graph size -> (backbone length, substitutions that each add one node)
NODE_COUNTS = {63: (61, 2), 64: (64, 0), 65: (64, 1), 128: (125, 3), 129: (126, 3)}


def node_count_windows():
    """A backbone plus layers that differ from it by substitutions only: each
    distinct (position, letter) adds exactly one node. The first substitution
    sits at position 0, so its node has no in-edge and a high id."""
    rng = random.Random(9000)
    wins = []
    for total, (blen, extra) in NODE_COUNTS.items():
        bb = _rand_seq(rng, blen)
        spots = [0, blen // 2, blen - 2][:extra]
        var = bb
        for p in spots:
            var = _sub_at(var, p)
        wins.append((f"count {total}", _window(rng, bb, [var, bb, var, var, bb])))
    return wins


def source_windows():
    """Layers that begin with a mismatch or with extra bases: their first
    node has in-degree 0 and an id behind the backbone's, so the sources lie
    in different 64-node blocks (node 0 in the first)."""
    rng = random.Random(9100)
    wins = []
    for blen in (130, 200):
        bb = _rand_seq(rng, blen)
        # node 0 stays a source: no layer puts a base in front of it
        lead_sub = _sub_at(bb, 0)                    # a second first node
        lead_sub2 = _sub_at(_sub_at(bb, 0, 2), 70)   # and a third
        lead_ins = 2 * _sub_at(bb[0], 0, 3) + lead_sub  # two bases before the second
        layers = [bb, lead_sub, _sub_at(bb, 100), lead_ins, lead_sub2, lead_sub, bb, lead_ins]
        wins.append((f"sources blen={blen}", _window(rng, bb, layers)))
    return wins


FAN_SITES = ((40, 5), (100, 3))  # (column, extra letters): out-degrees 10 and 8
FAN_MOTIF = "ACGTNA"             # backbone at column - 1 .. column + 4
FAN_LETTERS = "TNRYK"
FAN_PLAIN = 130                  # a plain substitution: out-degree 2 before it


def fan_window():
    """A node with 10 out-edges and one with exactly 8. At each site the
    backbone reads A|CGTN|A from column - 1. Four layers delete 1..4 bases
    starting at the column: the kept bases G, T, N, A are pairwise different,
    so each can only sit on its own node, and the node before the column
    gains the edges to them (1 + 4 out-edges). The later layers put another
    letter at the column. With the edge A -> G in the graph, inserting that
    letter between A and G costs one gap (-4) where a mismatch on C costs -5,
    so every such letter becomes a node of its own behind A, not a ring
    partner of C: one more out-edge each. The letters are none of A, C, G, so
    no insertion can slide. The read-back graph is asserted to have the
    degrees (test_out_degrees). Two layers also carry one substitution far
    behind both sites, for a node with exactly two out-edges."""
    rng = random.Random(9200)
    bb = list(_rand_seq(rng, 160))
    for col, _ in FAN_SITES:
        bb[col - 1:col + 5] = FAN_MOTIF
    bb = "".join(bb)
    layers = []
    for t in range(9):
        seq = list(bb)
        if t in (4, 5):
            seq[FAN_PLAIN] = "ACGT"[("ACGT".index(bb[FAN_PLAIN]) + 1) % 4]
        # right to left, so that a deletion does not shift the other site
        for col, extra in sorted(FAN_SITES, reverse=True):
            if t < 4:
                del seq[col:col + t + 1]
            elif t - 4 < extra:
                seq[col] = FAN_LETTERS[t - 4]
        layers.append("".join(seq))
    return ("fan out-degrees", _window(rng, bb, layers))


def variant_windows():
    """Longest layer <= 320, 321..575 (the mid variant, 1535-node cap) and
    >= 576 columns; substitutions and indels, so the graphs have bubbles."""
    rng = random.Random(9300)
    wins = []
    for tag, blen, lo, hi in (("narrow", 300, 0, 320), ("mid", 450, 321, 575),
                              ("full", 590, 576, 1023)):
        bb = _rand_seq(rng, blen)
        layers = [_mutate(rng, bb, 0.03, 0.03, 0.03) for _ in range(7)]
        layers.append(bb + _rand_seq(rng, 6) if tag == "full" else bb)
        assert lo <= max(len(s) for s in layers + [bb]) <= hi, tag
        wins.append((f"variant {tag}", _window(rng, bb, layers)))
    return wins


def all_cases():
    return node_count_windows() + source_windows() + [fan_window()] + variant_windows()


def kahn_fifo(edges):
    """The reference order: sources by ascending id, then FIFO, every node's
    out-edges in list order."""
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


@pytest.fixture(scope="module")
def consensus_batch(racon):
    """One CPU and one GPU run over every window."""
    cases = all_cases()
    windows = [w for _, w in cases]
    for tag, w in cases:
        assert 64 <= len(w[0][0]) <= 600 or tag == "count 63", tag
    return cases, racon.poa_windows_cpu(windows), racon.poa_windows_gpu(windows)


@pytest.fixture(scope="module")
def batch(racon, consensus_batch):
    """The same windows with one graph read-back and the CPU node counts."""
    cases, cpu, gpu = consensus_batch
    windows = [w for _, w in cases]
    graphs = racon.poa_window_graph_gpu(windows)
    counts = racon.poa_window_node_counts(windows)
    return cases, cpu, gpu, graphs, counts


def test_consensus_matches_cpu(consensus_batch):
    cases, cpu, gpu = consensus_batch
    for (tag, _), c, g in zip(cases, cpu, gpu):
        assert c[1], f"{tag}: the CPU engine did not polish the window"
        assert g[1], f"{tag}: GPU window failed over to the CPU"
        assert g == c, (tag, c[0], g[0])


def test_rank_is_the_kahn_fifo_order(batch):
    """rank[order[r]] == r for the FIFO order recomputed from the read-back
    adjacency, for every window; the graph has the CPU engine's node count."""
    cases, _, _, graphs, counts = batch
    for (tag, _), (status, rank, edges), count in zip(cases, graphs, counts):
        assert status == 0, (tag, status)
        assert len(rank) == len(edges) == count, (tag, len(rank), count)
        order = kahn_fifo(edges)
        assert len(order) == len(rank), f"{tag}: the read-back graph has a cycle"
        bad = [r for r, node in enumerate(order) if rank[node] != r]
        assert bad == [], (tag, bad[:8])


def test_node_counts_straddle_the_seed_blocks(batch):
    cases, _, _, graphs, _ = batch
    got = {tag: len(g[1]) for (tag, _), g in zip(cases, graphs) if tag.startswith("count")}
    assert got == {f"count {n}": n for n in NODE_COUNTS}


def test_sources_in_different_blocks(batch):
    cases, _, _, graphs, _ = batch
    seen = 0
    for (tag, _), (_, rank, edges) in zip(cases, graphs):
        if not tag.startswith("sources"):
            continue
        seen += 1
        targets = {v for row in edges for v in row}
        sources = [i for i in range(len(edges)) if i not in targets]
        assert len(sources) >= 3 and sources[0] == 0, (tag, sources)
        assert len({i // 64 for i in sources}) >= 2, (tag, sources)
        # sources are popped first, by ascending id
        assert [rank[i] for i in sources] == list(range(len(sources))), (tag, sources)
    assert seen == 2


def test_out_degrees(batch):
    """0, 1, 2, exactly 8 and 10 out-edges, asserted on the read-back graph."""
    cases, _, _, graphs, _ = batch
    k = [t for t, _ in cases].index("fan out-degrees")
    edges = graphs[k][2]
    degrees = [len(row) for row in edges]
    assert {0, 1, 2, 8, 10} <= set(degrees), sorted(set(degrees))
    assert degrees[FAN_SITES[0][0] - 1] == 10 and degrees[FAN_SITES[1][0] - 1] == 8
    assert degrees[FAN_PLAIN - 1] == 2


def test_one_window_per_ring_variant(batch):
    cases, _, gpu, graphs, _ = batch
    for tag, lo, hi in (("variant narrow", 1, 320), ("variant mid", 321, 575),
                        ("variant full", 576, 1023)):
        k = [t for t, _ in cases].index(tag)
        assert lo <= max(len(l[0]) for l in cases[k][1]) <= hi
        assert gpu[k][1] and graphs[k][0] == 0, tag
        assert len(graphs[k][1]) > len(cases[k][1][0][0]), tag  # the graph grew


def test_order_independence(racon, batch):
    """The batch reversed and shuffled gives identical consensus, ranks and
    adjacency per window: the LDS that the phases of a layer share leaks
    nothing from one window, or from one phase, into the next."""
    cases, _, gpu, graphs, _ = batch
    windows = [w for _, w in cases]
    n = len(windows)
    perm = list(range(n))
    random.Random(9400).shuffle(perm)
    for order in (list(range(n))[::-1], perm):
        got = racon.poa_windows_gpu([windows[k] for k in order])
        got_graphs = racon.poa_window_graph_gpu([windows[k] for k in order])
        assert [cases[k][0] for j, k in enumerate(order) if got[j] != gpu[k]] == []
        assert [cases[k][0] for j, k in enumerate(order) if got_graphs[j] != graphs[k]] == []


def test_hook_refuses_windows_without_a_slab(racon):
    """A window the device would not run (fewer than 3 layers) gets no slab:
    the read-back refuses the whole call."""
    rng = random.Random(9500)
    bb = _rand_seq(rng, 64)
    thin = [(bb, _qual(rng, 64), 0, 0), (bb, _qual(rng, 64), 0, 63)]
    with pytest.raises(RuntimeError):
        racon.poa_window_graph_gpu([all_cases()[0][1], thin])
