"""Parity tests for the lane-parallel add_alignment_d of the HIP POA kernel.

The kernel threads a layer's alignment into the graph 64 sequence positions
at a time (src/hip/poa_kernel.hip: sweep A resolves every position to a node
id with a ballot/popcount prefix sum, sweep B adds the edge between each
consecutive pair). The shapes here are the smallest at which that blocking
can go wrong: layer lengths around the 64-position blocks, edits at the block
seam, layers that add no node or a node at every position, aligned rings up
to and past their capacity, partial layers, and the node cap reached in the
middle of a block.

Reference: poa_windows_cpu on identical inputs; consensus string and polished
flag must both be equal. Every base carries its own quality, so the edge
weights differ and the heaviest-bundle walk has no uniform-weight tie
(docs/PARITY.md); one test repeats windows without layer qualities for the
unit-weight path. Windows that must leave the device (ring or node overflow)
assert the fallback itself.
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
# input builders (copied from test_gpu_kernel_edges.py, plus qualities/spans)
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
    """Per-base qualities with weights 1..93 (never the all-zero-weight graph
    the device refuses)."""
    return "".join(chr(34 + rng.randrange(93)) for _ in range(n))


def _window(rng, bb, layers, with_qual=True):
    """Window in differ form. A layer is a sequence (spanning the backbone)
    or (sequence, begin, end) with the pipeline's inclusive end."""
    blen = len(bb)
    out = [(bb, _qual(rng, blen) if with_qual else "!" * blen, 0, 0)]
    for item in layers:
        seq, begin, end = item if isinstance(item, tuple) else (item, 0, blen - 1)
        assert seq, "empty layer"
        out.append((seq, _qual(rng, len(seq)) if with_qual else "", begin, end))
    assert 3 <= len(out) - 1 <= 12
    return out


def _sub_at(seq, pos, shift=1):
    """seq with the base at pos replaced by the shift-th next letter."""
    pos %= len(seq)
    return seq[:pos] + "ACGT"[("ACGT".index(seq[pos]) + shift) % 4] + seq[pos + 1:]


BLOCK_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129)


def block_boundary_windows():
    """Layers of exactly L bases against a backbone of max(L, 64): once with
    substitutions only (the path is one diagonal, new nodes where a layer
    differs) and once with indels. L == 1 is the layer that adds no edge and
    no coverage; 64/65 puts the pair that straddles two blocks at its first
    possible position."""
    rng = random.Random(8000)
    wins = []
    for L in BLOCK_LENGTHS:
        blen = max(L, 64)
        bb = _rand_seq(rng, blen)
        if L <= 2:
            # short layers ride along with six ordinary ones; each sits on
            # its own span of two unequal nodes, where the one-base layer
            # (a match on the first or on the second node) has no
            # equal-score twin
            at = 30
            while bb[at] == bb[at + 1] or bb[at + 2] == bb[at + 3]:
                at += 1
            layers = [_mutate(rng, bb, 0.04, 0.0, 0.0) for _ in range(6)]
            layers[2:2] = [(bb[at:at + L], at, at + 1), (bb[at + 4 - L:at + 4], at + 2, at + 3)]
            wins.append((f"block sub L={L}", _window(rng, bb, layers)))
            continue
        cut = blen // 2
        src = bb if L == blen else bb[:cut] + bb[cut + 1:]
        assert len(src) == L
        layers = [_mutate(rng, src, 0.05, 0.0, 0.0) for _ in range(6)]
        assert all(len(s) == L for s in layers)
        wins.append((f"block sub L={L}", _window(rng, bb, layers)))
        layers = []
        while len(layers) < 6:
            s = _mutate(rng, src, 0.02, 0.03, 0.03)
            if len(s) >= L:
                layers.append(s[:L])
        wins.append((f"block indel L={L}", _window(rng, bb, layers)))
    return wins


def edit_windows():
    """One edit carried by five of seven layers of a 130-base window, so the
    consensus depends on the nodes, edges and weights the edit adds."""
    rng = random.Random(8100)
    wins = []

    def window(tag, edit):
        bb = _rand_seq(rng, 130)
        edited = edit(bb)
        layers = [edited, bb, edited, edited, bb, edited, edited]
        wins.append((tag, _window(rng, bb, layers)))

    for pos in (0, 63, 64, -1):
        window(f"edit mismatch at {pos}", lambda bb, pos=pos: _sub_at(bb, pos))
    # five inserted bases occupy layer positions 62..66: new -> new edges on
    # both sides of the block seam
    window("edit insertion 62..66", lambda bb: bb[:62] + _rand_seq(rng, 5) + bb[62:])
    # five deleted backbone bases: graph-only path entries at the seam
    window("edit deletion 62..66", lambda bb: bb[:62] + bb[67:])
    # a mismatch on either side of the seam plus an insertion ending on it
    window("edit mixed at seam",
           lambda bb: _sub_at(_sub_at(bb[:60] + _rand_seq(rng, 3) + bb[60:], 63), 64, 2))
    return wins


def prefix_sum_windows():
    """No new node at all (every ballot is zero) and a new node at every
    position of a 130-base layer (the running base crosses two blocks)."""
    rng = random.Random(8200)
    bb = _rand_seq(rng, 130)
    wins = [("prefix all match", _window(rng, bb, [bb] * 4))]
    ac = _rand_seq(rng, 130, "AC")
    gt = _rand_seq(rng, 130, "GT")
    # first GT layer: 130 new nodes; the later ones find them as ring partners
    wins.append(("prefix all new", _window(rng, ac, [gt, ac, gt, gt, ac])))
    wins.append(("prefix all new, minority", _window(rng, ac, [gt, ac, ac, gt, ac])))
    return wins


RING_COLUMN = 70


def ring_windows():
    """[0] a third layer repeats the second layer's mismatch; [1] A/C/G/T/N at
    one column fills the ring of four partners; [2] a sixth symbol at that
    column overflows it and the window goes to the CPU."""
    rng = random.Random(8300)
    wins = []
    bb = _rand_seq(rng, 130)
    var = _sub_at(bb, RING_COLUMN)
    wins.append(("ring partner reuse", _window(rng, bb, [bb, var, var, bb, var, var])))

    def column(symbols):
        layers = []
        for s in symbols:
            layer = bb[:RING_COLUMN] + s + bb[RING_COLUMN + 1:]
            layers += [layer, layer]  # the repeat resolves to the partner
        return layers

    others = [c for c in "ACGT" if c != bb[RING_COLUMN]]
    wins.append(("ring full", _window(rng, bb, column(others + ["N"]))))
    wins.append(("ring overflow", _window(rng, bb, column(others + ["N", "R"]))))
    return wins


def partial_layer_windows():
    """Layers whose backbone span starts and ends mid-window: the path starts
    at a virtual start row and ends at the span's end rank. The 150-base
    window sends every layer through the subgraph path, the 200-base one
    mixes it with window-spanning layers."""
    rng = random.Random(8400)
    wins = []
    for blen, spans in ((150, ((0, 149), (37, 120), (0, 149), (64, 149), (0, 63), (10, 140),
                               (0, 149), (60, 68), (20, 128))),
                        (200, ((0, 199), (37, 150), (0, 199), (64, 199), (0, 100), (50, 128),
                               (0, 199), (1, 198), (127, 192)))):
        bb = _rand_seq(rng, blen)
        layers = [(_mutate(rng, bb[b:e + 1], 0.03, 0.02, 0.02) or bb[b], b, e)
                  for b, e in spans]
        wins.append((f"partial blen={blen}", _window(rng, bb, layers)))
    return wins


def coverage_window():
    """100 bases; three spanning layers, five over 20..79 and two one-base
    layers on the first and last two nodes. Coverage floor (11 - 1) / 2 = 5;
    the ends sit at 1 + 3 = 4 and are trimmed, so one stray coverage count
    from a one-base layer (which has no edge and must count nowhere) or a
    lost one inside 20..79 moves the trimmed ends."""
    rng = random.Random(8500)
    bb = _rand_seq(rng, 100)
    while bb[0] == bb[1] or bb[98] == bb[99]:
        bb = _rand_seq(rng, 100)
    layers = [_mutate(rng, bb, 0.03, 0.0, 0.0) for _ in range(3)]
    layers += [(_mutate(rng, bb[20:80], 0.03, 0.0, 0.0), 20, 79) for _ in range(5)]
    layers.insert(2, (bb[0], 0, 1))
    layers.insert(6, (bb[99], 98, 99))
    return ("coverage trim", _window(rng, bb, layers))


def all_cases():
    cases = block_boundary_windows() + edit_windows() + prefix_sum_windows()
    cases += ring_windows() + partial_layer_windows() + [coverage_window()]
    return cases


FAILS_OVER = ("ring overflow",)


@pytest.fixture(scope="module")
def main_batch(racon):
    """One CPU and one GPU run (trim=True, tgs=True) over every window."""
    cases = all_cases()
    windows = [w for _, w in cases]
    for tag, w in cases:
        assert 64 <= len(w[0][0]) <= 200, tag
    cpu = racon.poa_windows_cpu(windows, trim=True, tgs=True)
    gpu = racon.poa_windows_gpu(windows, trim=True, tgs=True)
    return cases, cpu, gpu


def _check(main_batch, prefix):
    cases, cpu, gpu = main_batch
    seen = 0
    for (tag, _), c, g in zip(cases, cpu, gpu):
        if not tag.startswith(prefix):
            continue
        seen += 1
        assert c[1], f"{tag}: the CPU engine did not polish the window"
        if tag in FAILS_OVER:
            assert g[1] is False, f"{tag}: the GPU window did not fail over"
            continue
        assert g[1], f"{tag}: GPU window failed over to the CPU"
        assert g == c, (tag, c[0], g[0])
    assert seen > 0


def test_block_boundaries(main_batch):
    """Layer lengths 1, 2, 63, 64, 65, 127, 128, 129."""
    _check(main_batch, "block")


def test_position_specific_edits(main_batch):
    """Mismatch at 0 / 63 / 64 / len-1, insertion and deletion runs across the
    block seam."""
    _check(main_batch, "edit")


def test_zero_and_maximal_prefix_sums(main_batch):
    _check(main_batch, "prefix")


def test_ring_partners_and_ring_overflow(racon, main_batch):
    """Partner reuse, a full ring, and a sixth symbol that must take the
    ring-overflow path to the CPU."""
    _check(main_batch, "ring")
    cases, cpu, _ = main_batch
    # test-input sanity: the CPU consensus of the reuse window carries the
    # variant, so it was decided by the reused node's edges
    tag, w = cases[[t for t, _ in cases].index("ring partner reuse")]
    assert w[2][0][RING_COLUMN] != w[0][0][RING_COLUMN]
    assert w[2][0][RING_COLUMN - 5:RING_COLUMN + 6] in cpu[[t for t, _ in cases].index(tag)][0]


def test_partial_layers(main_batch):
    _check(main_batch, "partial")


def test_coverage_decides_trimmed_ends(main_batch):
    """trim=True, tgs=True: the coverage output (nseq plus ring partners)
    decides the trimmed ends."""
    _check(main_batch, "coverage")
    cases, cpu, _ = main_batch
    k = [t for t, _ in cases].index("coverage trim")
    # test-input sanity: the ends really are trimmed on the CPU
    assert 55 <= len(cpu[k][0]) <= 65, len(cpu[k][0])


def test_unit_weights_without_qualities(racon):
    """The same shapes without layer qualities (every weight 1, backbone 0):
    substitution-only windows at the block lengths, whose majority is clear
    without weights, and the all-match / all-new windows."""
    rng = random.Random(8600)
    cases = []
    for L in (64, 65, 129, 200):
        bb = _rand_seq(rng, L)
        layers = [_mutate(rng, bb, 0.04, 0.0, 0.0) for _ in range(12)]
        cases.append((f"unit sub L={L}", _window(rng, bb, layers, with_qual=False)))
    bb = _rand_seq(rng, 130)
    cases.append(("unit all match", _window(rng, bb, [bb] * 4, with_qual=False)))
    ac, gt = _rand_seq(rng, 130, "AC"), _rand_seq(rng, 130, "GT")
    cases.append(("unit all new", _window(rng, ac, [gt, gt, ac, gt, gt], with_qual=False)))
    windows = [w for _, w in cases]
    cpu = racon.poa_windows_cpu(windows)
    gpu = racon.poa_windows_gpu(windows)
    for (tag, _), c, g in zip(cases, cpu, gpu):
        assert c[1], tag
        assert g[1], f"{tag}: GPU window failed over to the CPU"
        assert g == c, (tag, c[0], g[0])


MID_NODE_CAP = 1535  # graph capacity of the variant for 321..575-column rows


def node_overflow_window():
    """400 x 'A' with layers of 400 x 'C', 'G', 'T', 'N'. No two share a base,
    every alignment is the plain diagonal (a mismatch beats two gaps), and
    each layer adds exactly 400 nodes whichever ring member the path runs
    through: 1200 nodes after 'G', so 'T' reaches the 1535-node cap at
    position 335 = 5 * 64 + 15, in the middle of its sixth block."""
    rng = random.Random(8700)
    return _window(rng, "A" * 400, ["C" * 400, "G" * 400, "T" * 400, "N" * 400])


def test_node_overflow_mid_block(racon):
    """The cap reached in the middle of a 64-position block: the window fails
    over to the CPU and its batch neighbours are unchanged. Also the
    insert-heavy window of test_poa_node_overflow_fails_over (500 bases, 30
    layers, 1800+ nodes under the same cap)."""
    rng = random.Random(8701)
    exact = node_overflow_window()
    bb = _rand_seq(rng, 500)
    heavy = [(bb, "!" * 500, 0, 0)]
    heavy += [(_mutate(rng, bb, 0.05, 0.10, 0.10), "", 0, 499) for _ in range(30)]
    counts = racon.poa_window_node_counts([exact, heavy])
    assert counts[0] == 2000, counts  # 5 x 400: the layer count argued above
    assert 1800 <= counts[1] and len(heavy) <= 96, counts
    assert all(321 <= max(len(l[0]) for l in w) <= 575 for w in (exact, heavy))
    assert (MID_NODE_CAP - 1200) % 64 not in (0, 63)
    assert all(ok for _, ok in racon.poa_windows_cpu([exact, heavy]))

    others = [w for _, w in edit_windows()[:2] + partial_layer_windows()]
    mixed = [others[0], exact, others[1], others[2], heavy, others[3]]
    got = racon.poa_windows_gpu(mixed)
    alone = racon.poa_windows_gpu(others)
    assert got[1][1] is False, "the window with the cap at position 335 did not fail over"
    assert got[4][1] is False, f"the insert-heavy window ({counts[1]} nodes) did not fail over"
    assert [got[0], got[2], got[3], got[5]] == alone
    assert all(ok for _, ok in alone)


def test_order_independence(racon, main_batch):
    """The same batch reversed and shuffled gives identical per-window
    results: nothing of one window's sweeps (LDS, slab arrays, the id array
    kept in aln_seq) leaks into the window that reuses its slot."""
    cases, _, gpu = main_batch
    windows = [w for _, w in cases]
    n = len(windows)
    rev = racon.poa_windows_gpu(windows[::-1])[::-1]
    assert rev == gpu, [cases[k][0] for k in range(n) if rev[k] != gpu[k]]
    perm = list(range(n))
    random.Random(8800).shuffle(perm)
    shuf = racon.poa_windows_gpu([windows[k] for k in perm])
    assert [cases[k][0] for j, k in enumerate(perm) if shuf[j] != gpu[k]] == []
