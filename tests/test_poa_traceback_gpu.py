"""Parity tests for the round-based traceback_d of the HIP POA kernel.

The traceback reads the predicted path 64 moves at a time (src/hip/
poa_kernel.hip: lane k takes the row reached after k diagonal moves through
in-edge 0, all lanes load their move byte in one round trip, the lanes before
the first other move record their node, that move is taken serially and the
next round starts behind it). The move bytes fix the path, so the result must
be the serial walk's. The shapes put the deviations at chosen distances: runs
of 15..129 diagonal moves between two edits (every power-of-two round depth
up to 64, plus and minus one), deviations back to back and across a round
boundary, layers with extra or missing leading bases (row 0 with columns
left, column 0 with rows left), partial layers (the virtual start row), and
layers with no deviation at all.

Reference: poa_windows_cpu on identical inputs; consensus string and polished
flag must both be equal. Every base carries its own quality, so the
heaviest-bundle walk has no uniform-weight tie (docs/PARITY.md). Windows are
64-600 bases with 3-16 layers; all are polished on the device except the
overflow windows, which must fail over. Everything runs with trim=True except
the windows whose layers start in front of the backbone (see main_batch).
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


def _no_repeat_seq(rng, n):
    """No two neighbours equal: a single-base insertion or deletion has one
    placement only, so the run lengths between edits are exact."""
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


def _window(rng, bb, layers, with_qual=True):
    blen = len(bb)
    out = [(bb, _qual(rng, blen) if with_qual else "!" * blen, 0, 0)]
    for item in layers:
        seq, begin, end = item if isinstance(item, tuple) else (item, 0, blen - 1)
        assert seq, "empty layer"
        out.append((seq, _qual(rng, len(seq)) if with_qual else "", begin, end))
    return out


def _other(ch, avoid=""):
    return next(c for c in "ACGT" if c != ch and c not in avoid)


def _sub_at(seq, pos):
    return seq[:pos] + _other(seq[pos]) + seq[pos + 1:]


def _ins_at(seq, pos, n=1):
    """n bases in front of seq[pos], the first unlike both neighbours."""
    first = _other(seq[pos], avoid=seq[pos - 1] if pos else "")
    run = [first]
    while len(run) < n:
        run.append(_other(run[-1], avoid=seq[pos] if len(run) == n - 1 else ""))
    return seq[:pos] + "".join(run) + seq[pos:]


def _del_at(seq, pos, n=1):
    return seq[:pos] + seq[pos + n:]


EDITS = {"sub": _sub_at, "ins": _ins_at, "del": _del_at}
MAJORITY = (1, 0, 1, 1, 0, 1, 1)  # which of seven layers carry the edits


def _majority_window(rng, bb, edited, partial=None):
    layers = [edited if m else bb for m in MAJORITY]
    if partial is not None:
        layers = [(s, *partial) for s in layers]
    return _window(rng, bb, layers)


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------

RUNS = (15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
TAIL = 20  # bases behind the second edit


def run_windows():
    """Two edits with exactly R matching bases between them, carried by five
    of seven layers. The walk comes from the end: TAIL diagonal moves, the
    second edit, a round that starts right behind it with R moves that hold,
    then the first edit. Substitutions are in the majority, so the later
    layers run through the new nodes and leave in-edge 0 behind them."""
    rng = random.Random(9600)
    wins = []
    for kind, edit in EDITS.items():
        for run in RUNS:
            blen = max(64, 12 + 1 + run + 1 + TAIL)
            bb = _no_repeat_seq(rng, blen)
            second = blen - TAIL - 1
            first = second - run - 1
            assert first >= 10
            # right to left: the first edit does not move the second
            edited = edit(edit(bb, second), first)
            wins.append((f"run {kind} R={run}", _majority_window(rng, bb, edited)))
    return wins


def adjacent_windows():
    """Deviations back to back (a round that accepts no move), and runs of
    five inserted / five deleted bases that begin 62..65 diagonal moves
    behind the layer's end, across the end of the first round."""
    rng = random.Random(9700)
    wins = []
    bb = _no_repeat_seq(rng, 130)
    wins.append(("adjacent two subs", _majority_window(rng, bb, _sub_at(_sub_at(bb, 71), 70))))
    wins.append(("adjacent sub+ins", _majority_window(rng, bb, _ins_at(_sub_at(bb, 70), 70))))
    wins.append(("adjacent del+sub", _majority_window(rng, bb, _del_at(_sub_at(bb, 69), 70))))
    for gap in (62, 63, 64, 65):
        bb = _no_repeat_seq(rng, 150)
        at = 150 - gap
        wins.append((f"adjacent ins5 {gap} from the end",
                     _majority_window(rng, bb, _ins_at(bb, at, 5))))
        wins.append((f"adjacent del5 {gap} from the end",
                     _majority_window(rng, bb, _del_at(bb, at - 5, 5))))
    return wins


def leading_windows():
    """Extra leading bases: the walk reaches row 0 with columns left, and the
    rest is filled in one step. Missing leading bases: it reaches column 0
    with rows left. Both also right behind a full round of 64."""
    rng = random.Random(9800)
    wins = []
    for blen in (100, 64):
        bb = _no_repeat_seq(rng, blen)
        for extra in (1, 3, 70):
            lead = _no_repeat_seq(rng, extra + 1)[:extra]
            if lead[-1] == bb[0]:
                lead = lead[:-1] + _other(bb[0], avoid=lead[-2:-1])
            wins.append((f"leading +{extra} blen={blen}", _majority_window(rng, bb, lead + bb)))
        for missing in (1, 3, 20):
            wins.append((f"leading -{missing} blen={blen}",
                         _majority_window(rng, bb, bb[missing:])))
    return wins


def partial_windows():
    """Layers on a span that starts mid-window: their first row is a virtual
    start row (edge sentinel 63 in the move byte). Spans of 63, 64, 65, 128
    and 129 bases copied from the backbone end exactly on a round boundary
    or next to one; the mutated ones deviate on the way."""
    rng = random.Random(9900)
    wins = []
    bb = _no_repeat_seq(rng, 200)
    for begin, n in ((37, 63), (37, 64), (37, 65), (50, 128), (50, 129), (136, 64)):
        end = begin + n - 1
        piece = bb[begin:end + 1]
        layers = [(piece, begin, end), bb, (piece, begin, end), (_sub_at(piece, n // 2), begin, end),
                  bb, (piece, begin, end)]
        wins.append((f"partial exact {begin}+{n}", _window(rng, bb, layers)))
    spans = ((0, 199), (37, 150), (0, 199), (64, 199), (0, 100), (50, 128), (0, 199), (1, 198),
             (127, 192))
    layers = [(_mutate(rng, bb[b:e + 1], 0.03, 0.02, 0.02), b, e) for b, e in spans]
    wins.append(("partial mutated", _window(rng, bb, layers)))
    return wins


def trivial_windows():
    """Layers equal to the backbone: no deviation at all."""
    rng = random.Random(10000)
    wins = []
    for blen in (64, 65, 130):
        bb = _rand_seq(rng, blen)
        wins.append((f"trivial blen={blen}", _window(rng, bb, [bb] * 4)))
    return wins


def mixed_windows():
    """Ordinary noisy windows of the three ring variants, 3..16 layers: paths
    through in-edges other than 0, up and left runs at random distances."""
    rng = random.Random(10100)
    wins = []
    for blen, depth in ((130, 16), (300, 3), (450, 12), (590, 8)):
        bb = _rand_seq(rng, blen)
        layers = [_mutate(rng, bb, 0.03, 0.03, 0.03) for _ in range(depth)]
        wins.append((f"mixed blen={blen}", _window(rng, bb, layers)))
    return wins


def all_cases():
    return (run_windows() + adjacent_windows() + leading_windows() + partial_windows() +
            trivial_windows() + mixed_windows())


@pytest.fixture(scope="module")
def main_batch(racon):
    """One CPU and one GPU run (trim=True, tgs=True) over every window."""
    cases = all_cases()
    windows = [w for _, w in cases]
    for tag, w in cases:
        assert 64 <= len(w[0][0]) <= 600 and 3 <= len(w) - 1 <= 16, tag
    cpu = racon.poa_windows_cpu(windows, trim=True, tgs=True)
    gpu = racon.poa_windows_gpu(windows, trim=True, tgs=True)
    # Bases in front of the backbone are compared untrimmed: with trim=True the
    # device's coverage trimming drops them and the CPU's keeps them, with or
    # without this traceback, which is not what these windows are about.
    untrimmed = [k for k, (tag, _) in enumerate(cases) if tag.startswith("leading +")]
    assert len(untrimmed) == 6
    sub = [windows[k] for k in untrimmed]
    for k, c, g in zip(untrimmed, racon.poa_windows_cpu(sub, trim=False, tgs=True),
                       racon.poa_windows_gpu(sub, trim=False, tgs=True)):
        cpu[k], gpu[k] = c, g
    return cases, cpu, gpu


def _check(main_batch, prefix):
    cases, cpu, gpu = main_batch
    seen = 0
    for (tag, _), c, g in zip(cases, cpu, gpu):
        if not tag.startswith(prefix):
            continue
        seen += 1
        assert c[1], f"{tag}: the CPU engine did not polish the window"
        assert g[1], f"{tag}: GPU window failed over to the CPU"
        assert g == c, (tag, c[0], g[0])
    return seen


@pytest.mark.parametrize("kind", sorted(EDITS))
def test_diagonal_runs_between_edits(main_batch, kind):
    """Runs of 15..129 matching bases between two substitutions, two
    single-base insertions, two single-base deletions."""
    assert _check(main_batch, f"run {kind}") == len(RUNS)


def test_back_to_back_deviations(main_batch):
    assert _check(main_batch, "adjacent") == 11


def test_leading_edits(main_batch):
    assert _check(main_batch, "leading") == 12
    # test-input sanity: the consensus keeps the extra bases, so the nodes
    # that the row-0 fill threads into the graph decide it
    cases, cpu, _ = main_batch
    for (tag, w), c in zip(cases, cpu):
        if tag.startswith("leading +"):
            assert len(c[0]) == len(w[1][0]) > len(w[0][0]), tag


def test_partial_layers(main_batch):
    assert _check(main_batch, "partial") == 7


def test_trivial_paths(main_batch):
    assert _check(main_batch, "trivial") == 3


def test_noisy_windows_of_every_variant(main_batch):
    assert _check(main_batch, "mixed") == 4


MID_NODE_CAP = 1535  # graph capacity of the variant for 321..575-column rows
RING_COLUMN = 70


def overflow_windows():
    """The fail-over shapes of test_poa_add_alignment_gpu.py: 400 x 'A' with
    layers of 400 x 'C', 'G', 'T', 'N' (2000 nodes against the 1535-node
    cap), an insert-heavy 500-base window of 30 layers (1800+ nodes), and a
    column with six symbols (a fifth ring partner)."""
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
    """Node and ring overflow: the windows fail over to the CPU and their
    batch neighbours are unchanged."""
    exact, heavy, ring = overflow_windows()
    counts = racon.poa_window_node_counts([exact, heavy])
    assert counts[0] == 2000 and counts[1] >= 1800, counts
    assert all(ok for _, ok in racon.poa_windows_cpu([exact, heavy, ring]))
    cases, _, _ = main_batch
    picks = ("run sub R=64", "adjacent ins5 64 from the end", "leading -3 blen=100",
             "partial mutated")
    others = [w for tag, w in cases if tag in picks]
    assert len(others) == 4
    mixed = [others[0], exact, others[1], ring, others[2], heavy, others[3]]
    got = racon.poa_windows_gpu(mixed)
    alone = racon.poa_windows_gpu(others)
    assert got[1][1] is False, "the 2000-node window did not fail over"
    assert got[3][1] is False, "the six-symbol column did not fail over"
    assert got[5][1] is False, f"the insert-heavy window ({counts[1]} nodes) did not fail over"
    assert [got[0], got[2], got[4], got[6]] == alone
    assert all(ok for _, ok in alone)


def test_order_independence(racon, main_batch):
    """The batch reversed gives identical per-window results."""
    cases, _, gpu = main_batch
    windows = [w for _, w in cases]
    rev = racon.poa_windows_gpu(windows[::-1], trim=True, tgs=True)[::-1]
    assert [cases[k][0] for k in range(len(cases))
            if rev[k] != gpu[k] and not cases[k][0].startswith("leading +")] == []
