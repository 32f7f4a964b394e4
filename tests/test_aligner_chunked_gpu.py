"""Shapes at which the lane aligner's word-wise sequence reads, register-held
Peq words and batched traceback can go wrong (src/hip/aligner_kernel.hip).

The kernel reads the sequence arena in aligned 8-byte words (Peq fill, target
codes, traceback), keeps the Peq words of a K = 4 diagonal band in registers
and shifts them when the band slides, and walks the traceback in batches of
columns fetched at the walk's row block. The shapes below sit on the edges of
those words, chunks, blocks and batches.

Expected values never come from the kernel under test:
  - the edit distance is racon.edit_distance (CPU);
  - every CIGAR consumes exactly n and m and costs exactly the distance;
  - where the whole matrix lies inside the band (n <= band) the exact CIGAR is
    that of a plain full-matrix DP here, walked back from (n, m) preferring
    the diagonal, then the target-consuming, then the query-consuming move;
  - breaking points equal breaking_points_from_cigar over the CIGAR that
    gpu_align returns (as in test_breaking_points_gpu.py);
  - the statuses of the pairs that may escape the band are the ones the build
    before this file's kernel change returned (PINNED_STATUS); the whole file
    passed on that build.
"""

import random
import re

import pytest

pytestmark = pytest.mark.gpu

EDGE_LENGTHS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]

# Status per tag under (diagonal, adaptive, retry) at band 256, recorded on
# the parent build: 0 ok, 1 band edge. Every pair not listed completes under
# every policy.
PINNED_STATUS = {
    "n=1000 m=8": (1, 1, 1),
    "n=700 m=3": (1, 1, 1),
    "n=3 m=700": (0, 0, 0),
    "300-base insertion": (1, 1, 1),
    "insertion run 200": (1, 1, 1),
    "insertion run 130": (0, 1, 0),
    "insertion run 200 ending at column 1": (1, 1, 1),
    "n=257 m=129": (0, 1, 0),
}
POLICIES = ["diagonal", "adaptive", "retry"]


@pytest.fixture(scope="module", autouse=True)
def require_gpu(racon):
    # torch is deliberately not imported (see test_gpu_kernel_edges.py)
    if racon.device_count() < 1:
        pytest.skip("no GPU on this host")


# --------------------------------------------------------------------------
# references
# --------------------------------------------------------------------------

def _sub(qc, tc):
    """The kernel's substitution cost: only A/C/G/T ever match."""
    return 0 if (qc == tc and qc in "ACGT") else 1


_DP_CACHE = {}


def dp_cigar(q, t):
    """(distance, CIGAR) of the full matrix, D(i, 0) = i and D(0, j) = j,
    walked back from (n, m): diagonal first, then left (D), then up (I)."""
    key = (q, t)
    if key in _DP_CACHE:
        return _DP_CACHE[key]
    n, m = len(q), len(t)
    rows = [list(range(m + 1))]
    for i in range(1, n + 1):
        prev = rows[-1]
        row = [i] * (m + 1)
        qc = q[i - 1]
        for j in range(1, m + 1):
            best = prev[j - 1] + _sub(qc, t[j - 1])
            left = row[j - 1] + 1
            up = prev[j] + 1
            if left < best:
                best = left
            if up < best:
                best = up
            row[j] = best
        rows.append(row)
    ops = []
    i, j = n, m
    while i > 0 and j > 0:
        d = rows[i][j]
        if rows[i - 1][j - 1] + _sub(q[i - 1], t[j - 1]) == d:
            ops.append("M")
            i -= 1
            j -= 1
        elif rows[i][j - 1] + 1 == d:
            ops.append("D")
            j -= 1
        else:
            assert rows[i - 1][j] + 1 == d
            ops.append("I")
            i -= 1
    ops.extend("I" * i)
    ops.extend("D" * j)
    ops.reverse()
    cigar = "".join(f"{len(run.group(0))}{run.group(0)[0]}"
                    for run in re.finditer(r"M+|I+|D+", "".join(ops)))
    _DP_CACHE[key] = (rows[n][m], cigar)
    return _DP_CACHE[key]


def cigar_walk(q, t, cigar):
    """(query bases, target bases, cost) a CIGAR of M / I / D runs covers."""
    assert re.fullmatch(r"(\d+[MID])+", cigar), cigar[:60]
    qi = ti = cost = 0
    for num, op in re.findall(r"(\d+)([MID])", cigar):
        num = int(num)
        if op == "M":
            cost += sum(_sub(q[qi + k], t[ti + k]) for k in range(num))
            qi += num
            ti += num
        elif op == "I":
            cost += num
            qi += num
        else:
            cost += num
            ti += num
    return qi, ti, cost


def _rand(rng, length, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(length))


def _mutate(rng, seq, rate):
    """Substitutions, insertions and deletions, each at `rate` per base."""
    out = []
    for ch in seq:
        r = rng.random()
        if r < rate:
            continue
        if r < 2 * rate:
            out.append(rng.choice("ACGT"))
        if r < 3 * rate:
            out.append(rng.choice([c for c in "ACGT" if c != ch]))
        else:
            out.append(ch)
    return "".join(out)


def _related(rng, t, n, rate=0.05):
    """A query of exactly n bases derived from t."""
    q = _mutate(rng, t, rate)
    return (q + _rand(rng, n))[:n]


def run_and_check(racon, cases, band=256, policy="diagonal", windows=(16, 64), pinned=None):
    """cases: (tag, query, target). One gpu_align call and one
    gpu_breaking_points call per window length over all of them. A pair
    completes (status 0) unless `pinned` says otherwise. Returns the gpu_align
    results."""
    pairs = [(q, t) for _, q, t in cases]
    res = racon.gpu_align(pairs, band_width=band, band_policy=policy)
    assert len(res) == len(cases)
    for (tag, q, t), (cigar, ed, status) in zip(cases, res):
        print(f"{policy} band {band} {tag}: status {status} distance {ed}")
    for (tag, q, t), (cigar, ed, status) in zip(cases, res):
        want_status = 0
        if pinned is not None and tag in pinned:
            want_status = pinned[tag][POLICIES.index(policy)]
        assert status == want_status, (tag, policy, status)
        if status != 0:
            assert cigar == "", (tag, policy)
            continue
        assert ed == racon.edit_distance(q, t), (tag, policy, "distance")
        assert cigar_walk(q, t, cigar) == (len(q), len(t), ed), (tag, policy, "cigar walk")
        if len(q) <= band and len(q) * len(t) <= 70000:
            assert (ed, cigar) == dp_cigar(q, t), (tag, policy, "exact cigar")
    t_begins = [(37 * k) % 200 for k in range(len(cases))]
    q_begins = [(13 * k) % 90 for k in range(len(cases))]
    for L in windows:
        got = racon.gpu_breaking_points(pairs, L, t_begins=t_begins, q_begins=q_begins,
                                        band_width=band, band_policy=policy)
        for (tag, q, t), (cigar, ed, status), g, tb, qb in zip(cases, res, got, t_begins, q_begins):
            want = []
            if status == 0:
                want = racon.breaking_points_from_cigar(cigar, L, tb, tb + len(t), qb)
            assert g[2] == status and g[1] == ed, (tag, policy, L, g[1:], (ed, status))
            assert g[0] == want, (tag, policy, L, g[0][:6], want[:6])
    return res


# --------------------------------------------------------------------------
# shapes
# --------------------------------------------------------------------------

def chunk_edge_cases():
    """Every edge length as n with itself and with two other edge lengths as
    m, so that each length occurs on both axes: 46 pairs, not the 400 of the
    product. n = 257 is five blocks at band 256 (one slide)."""
    rng = random.Random(9100)
    cases = []
    for k, n in enumerate(EDGE_LENGTHS):
        for m in (n, EDGE_LENGTHS[(k * 7 + 3) % 20], EDGE_LENGTHS[(k * 3 + 11) % 20]):
            if not (n + 1) // 2 <= m <= 2 * n and (n > 64 or m > 64):
                continue  # far off the diagonal: left to the slide cases
            t = _rand(rng, m)
            cases.append((f"n={n} m={m}", _related(rng, t, n), t))
    return cases


def non_acgt_cases():
    """Lengths are multiples of 16, so every sequence starts a 16-byte chunk
    of the arena and offsets within a sequence are offsets within a chunk."""
    rng = random.Random(9200)
    cases = []
    t0 = _rand(rng, 128)
    q0 = "".join(rng.choice("ACGT") if rng.random() < 0.04 else c for c in t0)
    for bad in ("N", "a", "t"):
        for offs in ((7,), (8,), (15,), (16,), (7, 8, 15, 16), (23, 24, 31, 32, 127)):
            t = list(t0)
            for o in offs:
                t[o] = bad
            cases.append((f"target {bad!r} at {offs}", q0, "".join(t)))
        for offs in ((63,), (64,), (62, 63, 64, 65), (127,)):
            q = list(q0)
            for o in offs:
                q[o] = bad
            cases.append((f"query {bad!r} at rows {offs}", "".join(q), t0))
    return cases


def ring_cases():
    rng = random.Random(9300)
    cases = []
    a = _rand(rng, 100, "ACG")
    b = _rand(rng, 100, "ACG")
    for run in (70, 130, 200):
        cases.append((f"insertion run {run}", a + "T" * run + b, a + b))
        cases.append((f"deletion run {run}", a + b, a + "T" * run + b))
        cases.append((f"insertion run {run} ending at column 1", a[0] + "T" * run + a[1:], a))
        cases.append((f"deletion run {run} ending at row 1", a, a[0] + "T" * run + a[1:]))
    body = _rand(rng, 200, "ACG")
    # three extra query bases at row 60: rows 64 and 128 are crossed at columns
    # 61 and 125; three missing ones: at columns 67 and 131
    cases.append(("insertion before a block boundary", body[:60] + "TTT" + body[60:], body))
    cases.append(("deletion before a block boundary", body[:60] + body[63:], body))
    cases.append(("indels before both boundaries",
                  body[:62] + "TT" + body[62:120] + body[125:], body))
    return cases


def slide_cases():
    rng = random.Random(9400)
    cases = []
    for n in (130, 300, 600):
        t = _rand(rng, n)
        cases.append((f"n=m={n} identical", t, t))
        q = _mutate(rng, t, 0.05 / 3)
        cases.append((f"n={len(q)} m={n} 5 % edits", q, t))
    return cases


def lopsided_cases():
    rng = random.Random(9500)
    return [(f"n={n} m={m}", _rand(rng, n), _rand(rng, m))
            for n, m in ((1000, 8), (700, 3), (3, 700))]


@pytest.mark.parametrize("policy", POLICIES)
def test_word_and_chunk_edges(racon, policy):
    """n and m on and around the 8- and 16-byte word, 64-row block and
    256-row band edges; the whole matrix is in band, so the CIGAR is exact."""
    cases = chunk_edge_cases()
    lengths_n = {len(q) for _, q, _ in cases}
    lengths_m = {len(t) for _, _, t in cases}
    assert lengths_n == set(EDGE_LENGTHS) and lengths_m == set(EDGE_LENGTHS)
    run_and_check(racon, cases, policy=policy, pinned=PINNED_STATUS)


def test_sequence_offsets(racon):
    """Query lengths through every residue mod 16 (targets too, at another
    phase): each target and the query after it start at every misalignment.
    Then fills of one 1-base pair: the arena's first byte is its last."""
    rng = random.Random(9600)
    cases = []
    for k in range(32):
        n = 33 + k
        m = 40 + (5 * k) % 16 + k // 16
        t = _rand(rng, m)
        cases.append((f"offset pair {k} n={n} m={m}", _related(rng, t, n), t))
    assert {len(q) % 16 for _, q, _ in cases} == set(range(16))
    assert {len(t) % 16 for _, _, t in cases} == set(range(16))
    run_and_check(racon, cases)
    run_and_check(racon, [("single match", "A", "A")])
    run_and_check(racon, [("single mismatch", "G", "T")])


@pytest.mark.parametrize("policy", POLICIES)
def test_non_acgt(racon, policy):
    """N and lowercase bases at offsets 7, 8, 15, 16 of a target chunk and at
    bits 63 / 64 of a query block match nothing. A pair with such a byte on
    both sides is refused (status 2): host and device would cost it
    differently (AlignerBatch::reserve_span)."""
    run_and_check(racon, non_acgt_cases(), policy=policy)
    rng = random.Random(9700)
    t = _rand(rng, 64)
    for bad in ("N", "g"):
        got = racon.gpu_align([(t[:-1] + bad, t[:-1] + bad), (t, t)], band_width=256,
                              band_policy=policy)
        assert got[0] == ("", -1, 2), got[0]
        assert got[1] == ("64M", 0, 0), got[1]


@pytest.mark.parametrize("policy", POLICIES)
def test_traceback_runs(racon, policy):
    """Vertical runs across one and several row blocks in one column,
    horizontal runs that leave windows without a match (window lengths 16 and
    64), indels that shift the block crossings off the diagonal, and runs that
    end at column 1 / row 1."""
    cases = ring_cases()
    res = run_and_check(racon, cases, policy=policy, pinned=PINNED_STATUS)
    if policy == "diagonal":
        for (tag, q, t), (cigar, _, _) in zip(cases, res):
            if tag.startswith("deletion run") and "row 1" not in tag and cigar:
                points = racon.breaking_points_from_cigar(cigar, 16, 0, len(t), 0)
                # test-input sanity: the run empties at least two whole windows
                assert len(points) // 2 <= -(-len(t) // 16) - 2, tag


def test_slides(racon):
    """One slide per 64 columns (n = m), identical and at 5 % edits."""
    run_and_check(racon, slide_cases())


@pytest.mark.parametrize("policy", POLICIES)
def test_several_blocks_per_column(racon, policy):
    """A query many times its target slides several blocks per column, and
    the reverse never slides. Statuses as recorded on the parent build; a
    completed pair holds the optimum."""
    run_and_check(racon, lopsided_cases(), policy=policy, pinned=PINNED_STATUS)


def _wave_cases(count, seed):
    rng = random.Random(seed)
    cases = []
    for k in range(count):
        m = 1 + (k * 599) // max(1, count - 1) if count > 3 else (5, 300, 77)[k]
        # interleave short and long so that every wave mixes them
        t = _rand(rng, m)
        q = _mutate(rng, t, 0.01) or "A"
        cases.append((f"pair {k} of {count} m={m}", q, t))
    rng.shuffle(cases)
    return cases


@pytest.mark.parametrize("count", [64, 65, 3])
def test_waves(racon, count):
    """64 pairs of 1 to 600 bases in one launch (short lanes coast while the
    long ones finish), one more than 64, and three (a single thin wave)."""
    run_and_check(racon, _wave_cases(count, 9800 + count), windows=(64,))


@pytest.mark.parametrize("band", [512, 1024])
def test_wider_bands(racon, band):
    """K = 8 and 16 keep the Peq gather but take their codes from the same
    word-wise target reads."""
    run_and_check(racon, chunk_edge_cases() + slide_cases() + ring_cases(), band=band,
                  windows=(64,))


@pytest.mark.parametrize("policy", POLICIES)
def test_one_escape_between_exact_neighbours(racon, policy):
    """A 300-base insertion leaves the 256 band; the pairs around it in the
    same wave are untouched."""
    rng = random.Random(9900)
    a, b = _rand(rng, 300, "ACG"), _rand(rng, 300, "ACG")
    n1, n2 = _rand(rng, 200), _rand(rng, 233)
    cases = [("neighbour before", _mutate(rng, n1, 0.02), n1),
             ("300-base insertion", a + "T" * 300 + b, a + b),
             ("neighbour after", _mutate(rng, n2, 0.02), n2)]
    run_and_check(racon, cases, policy=policy, pinned=PINNED_STATUS)
