"""Kernel-edge parity tests for the HIP Myers aligner and the HIP POA kernel.

The shapes here are the ones the kernels branch on: 64-row block and band
boundaries, the 16/64 lanes-per-wave switch, the five POA kernel variants'
routing thresholds, windows shorter than every margin, the capacity
contracts, and the rare-numerics paths (non-ACGT letters, quality weights,
score sets up to the int16 guard).

References: a plain NumPy edit-distance DP (np_edit_distance, itself checked
against racon.edit_distance in test_edge_refs.py on the CPU) for the aligner,
and poa_windows_cpu on identical inputs for the POA kernel.

Aligner band contract (derived from btop_of in aligner_kernel.hip): the band
at column j covers the K 64-row blocks [cb - K/2, cb + K/2) around
cb = floor(j*n/m) / 64, i.e. every row i with |i - j*n/m| <= 32*K - 63. A
global path of cost C never leaves |i - j*n/m| <= C (write i - j*n/m as
a*(1 - j/m) - b*j/m with a, b the net indels before / after the cell and
|a| + |b| <= C). In-band scores are upper bounds that are exact along any
path that stays in band, and the traceback only ever steps to a cell whose
stored score equals the true optimum, so with 0.5 <= n/m <= 2 (the band
center moves at most 2 rows per column) every pair whose optimum is at most
    BAND_EXACT_BOUND(K) = 64*(K/2 - 1) - 8
must come back status 0 with the optimal distance. Beyond the bound a result
is either a fallback (status != 0, empty CIGAR) or a valid CIGAR whose cost
equals the reported distance, which may then exceed the optimum.
"""

import random
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def require_gpu(racon):
    # NOTE: torch is deliberately not imported here — torch bundles its own
    # HIP runtime and loading it after _racon (system ROCm) aborts the
    # process. bench.py imports torch first, which is safe.
    if racon.device_count() < 1:
        pytest.skip("no GPU on this host")


# --------------------------------------------------------------------------
# reference helpers (CPU-only; exercised by test_edge_refs.py)
# --------------------------------------------------------------------------

def np_edit_distance(a, b):
    """Unit-cost global edit distance over byte equality (N matches N)."""
    if len(a) > len(b):
        a, b = b, a  # fewer python-level rows; the distance is symmetric
    av = np.frombuffer(a.encode(), dtype=np.uint8)
    bv = np.frombuffer(b.encode(), dtype=np.uint8)
    m = len(bv)
    idx = np.arange(m + 1, dtype=np.int32)
    prev = idx.copy()
    cur = np.empty(m + 1, dtype=np.int32)
    for i in range(len(av)):
        cur[0] = i + 1
        np.minimum(prev[:-1] + (bv != av[i]).astype(np.int32), prev[1:] + 1, out=cur[1:])
        # left chain: cur[j] = min_k<=j (cur[k] + (j - k))
        cur = np.minimum.accumulate(cur - idx) + idx
        prev, cur = cur, prev
    return int(prev[m])


_CIGAR_RE = re.compile(r"(\d+)([A-Za-z=])")


def replay_cigar(q, t, cigar):
    """Walks a CIGAR over (q, t): returns (q_used, t_used, cost) with M
    costing 1 per unequal byte pair and I/D 1 per base. Raises ValueError on
    anything but M/I/D runs or on a run that overshoots either sequence."""
    if "".join(n + op for n, op in _CIGAR_RE.findall(cigar)) != cigar:
        raise ValueError(f"malformed CIGAR: {cigar[:40]!r}")
    qi = ti = cost = 0
    for num, op in _CIGAR_RE.findall(cigar):
        num = int(num)
        if op == "M":
            if qi + num > len(q) or ti + num > len(t):
                raise ValueError("M run overshoots a sequence")
            cost += sum(1 for k in range(num) if q[qi + k] != t[ti + k])
            qi += num
            ti += num
        elif op == "I":
            cost += num
            qi += num
        elif op == "D":
            cost += num
            ti += num
        else:
            raise ValueError(f"CIGAR op {op!r} is not one of M/I/D")
    return qi, ti, cost


# --------------------------------------------------------------------------
# input builders (deterministic; shared with test_edge_refs.py)
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


def _fit_length(rng, seq, m):
    """seq cut or padded with random bases at its end to exactly m bytes."""
    if len(seq) >= m:
        return seq[:m]
    return seq + _rand_seq(rng, m - len(seq))


BANDS = (256, 512, 1024)  # -> K = 4, 8, 16 blocks


def band_exact_bound(K):
    return 64 * (K // 2 - 1) - 8


def aligner_boundary_pairs(band):
    """§1a: (tag, query, target) around the 64-row block and band edges."""
    K = band // 64
    rng = random.Random(1000 + band)
    pairs = []
    for n in (1, 2, 63, 64, 65, 127, 128, 129, 64 * K - 1, 64 * K, 64 * K + 1,
              2 * 64 * K + 1):
        q = _rand_seq(rng, n)
        for m in (n - 1, n, n + 1):
            if m < 1:
                continue
            # 3% error in all, so the optimum stays under band_exact_bound(4)
            t = _fit_length(rng, _mutate(rng, q, 0.01, 0.01, 0.01), m)
            pairs.append((f"mut n={n} m={m}", q, t))
        pairs.append((f"identical n={n}", q, q))
        pairs.append((f"mismatch n={n} m={n}", "A" * n, "C" * n))
        pairs.append((f"mismatch n={n} m={n + 1}", "A" * n, "C" * (n + 1)))
        pairs.append((f"homopolymer n={n}", "A" * n, "A" * (n + 5)))
    q = _rand_seq(rng, 65)
    pairs.append(("n=65 m=1", q, q[10]))
    return pairs


def _deletion_pair(rng, d, where, m=3000):
    """Target of m bases; query = target minus one d-base block (at the
    start, middle or end) plus 10 substitutions elsewhere."""
    t = _rand_seq(rng, m)
    at = {"start": 0, "middle": (m - d) // 2, "end": m - d}[where]
    q = list(t[:at] + t[at + d:])
    for pos in rng.sample(range(len(q)), 10):
        q[pos] = rng.choice([c for c in "ACGT" if c != q[pos]])
    return "".join(q), t


def band_contract_exact_pairs(band):
    """§1d must-be-exact set: optimum <= d + 10 <= band_exact_bound(K)."""
    rng = random.Random(2000 + band)
    ds = {256: (8, 40), 512: (150,), 1024: (400,)}[band]
    return [(f"del d={d}", *_deletion_pair(rng, d, "middle")) for d in ds]


def band_contract_escape_pairs():
    """§1d escape set (band 256, K = 4): optimum far above the bound."""
    rng = random.Random(2999)
    pairs = []
    for where in ("middle", "start", "end"):
        for d in (300, 600):
            pairs.append((f"escape d={d} {where}", *_deletion_pair(rng, d, where)))
    pairs.append(("skew 3000x40", _rand_seq(rng, 3000), _rand_seq(rng, 40)))
    pairs.append(("skew 40x3000", _rand_seq(rng, 40), _rand_seq(rng, 3000)))
    return pairs


def mixed_wave_pairs():
    """§1b: two long pairs and ~40 one-to-five-column targets in one batch,
    so short lanes share a wave with a long mmax. Errors are kept at 1% so
    the long pairs' optimum (~60) is under band_exact_bound(8) = 184; the
    short queries (n <= 70) fit inside the K-block band entirely."""
    rng = random.Random(3000)
    pairs = []
    for n in (6000, 3000):
        t = _rand_seq(rng, n)
        pairs.append((f"long n~{n}", _mutate(rng, t, 0.005, 0.0025, 0.0025), t))
    for k in range(40):
        m = 1 + k % 5
        n = 1 + (k * 7) % 70
        pairs.append((f"short n={n} m={m}", _rand_seq(rng, n), _rand_seq(rng, m)))
    return pairs


def lane_packing_pairs():
    """§1c: 16 400 pairs, n in 1..130, 5% error — crosses the na >= 16384
    switch to 64 alignments per wave and leaves a partial last wave."""
    rng = random.Random(4000)
    pairs = []
    for k in range(16400):
        t = _rand_seq(rng, 1 + (k * 37) % 130)
        q = _mutate(rng, t, 0.05, 0.05, 0.05) or rng.choice("ACGT")
        pairs.append((q, t))
    return pairs


def assert_sound(racon, tag, q, t, result, optimum):
    """Soundness of one status-0 aligner result."""
    cigar, ed, status = result
    assert status == 0, tag
    q_used, t_used, cost = replay_cigar(q, t, cigar)  # raises unless M/I/D only
    assert (q_used, t_used) == (len(q), len(t)), (tag, q_used, t_used)
    assert cost == ed, (tag, cost, ed)
    assert ed >= optimum, (tag, ed, optimum)


def assert_exact(racon, tag, q, t, result, optimum):
    assert_sound(racon, tag, q, t, result, optimum)
    assert result[1] == optimum, (tag, result[1], optimum)


# --------------------------------------------------------------------------
# 1. aligner
# --------------------------------------------------------------------------

@pytest.mark.parametrize("band", BANDS)
def test_aligner_block_and_band_boundaries(racon, band):
    """§1a + §1d: every boundary pair and every pair whose optimum is under
    the band bound is exact; escape-set results are fallbacks or sound."""
    K = band // 64
    exact = aligner_boundary_pairs(band) + band_contract_exact_pairs(band)
    n_contract = len(band_contract_exact_pairs(band))
    escape = band_contract_escape_pairs() if band == 256 else []
    allp = exact + escape
    res = racon.gpu_align([(q, t) for _, q, t in allp], band_width=band)
    assert len(res) == len(allp)

    for k, ((tag, q, t), r) in enumerate(zip(exact, res)):
        opt = np_edit_distance(q, t)
        if k >= len(exact) - n_contract:
            assert opt <= band_exact_bound(K), (tag, opt)  # test-input sanity
        assert_exact(racon, f"band {band}: {tag}", q, t, r, opt)

    non_optimal = fallbacks = 0
    for (tag, q, t), r in zip(escape, res[len(exact):]):
        opt = np_edit_distance(q, t)
        if r[2] != 0:
            assert r[0] == "", tag
            fallbacks += 1
            continue
        assert_sound(racon, tag, q, t, r, opt)
        if r[1] > opt:
            non_optimal += 1
        print(f"escape {tag}: status 0, distance {r[1]}, optimum {opt}")
    if escape:
        # informational (maintainer-facing), not a pass condition
        print(f"escape set: {len(escape)} pairs, {fallbacks} fallbacks, "
              f"{non_optimal} status-0 results above the optimum")


def test_aligner_mixed_wave(racon):
    """§1b: lanes that finish after 1-5 columns coast to a 6000-column mmax."""
    pairs = mixed_wave_pairs()
    res = racon.gpu_align([(q, t) for _, q, t in pairs])
    for (tag, q, t), r in zip(pairs, res):
        assert_exact(racon, tag, q, t, r, np_edit_distance(q, t))


def test_aligner_64_lane_packing(racon):
    """§1c: the flagship 64-lanes-per-wave packing with a partial last wave."""
    pairs = lane_packing_pairs()
    assert len(pairs) >= 16384 and len(pairs) % 64 != 0
    res = racon.gpu_align(pairs)
    assert len(res) == len(pairs)
    for k, ((q, t), r) in enumerate(zip(pairs, res)):
        # n <= 130 < 64*K: the band holds the whole matrix, nothing escapes
        assert_exact(racon, f"pair {k}", q, t, r, racon.edit_distance(q, t))


def nonacgt_pairs():
    """§1f: N runs in the same place, on one side only, and all-N."""
    rng = random.Random(5000)
    a = _rand_seq(rng, 300)
    b = _mutate(rng, a, 0.02, 0.02, 0.02)
    return [
        ("issue example", "ACGTNNNNACGT", "ACGTNNNNACGT"),
        ("N run both", a[:100] + "N" * 20 + a[100:], a[:100] + "N" * 20 + a[100:]),
        ("N run both, mutated", a[:100] + "N" * 20 + a[100:], b[:100] + "N" * 20 + b[100:]),
        ("N in query only", a[:150] + "NNN" + a[153:], a),
        ("N in target only", a, a[:150] + "NNN" + a[153:]),
        ("single N both", a[:64] + "N" + a[65:], a[:64] + "N" + a[65:]),
        ("all N", "N" * 70, "N" * 70),
        ("all N unequal", "N" * 70, "N" * 64),
        ("other IUPAC", "ACGTRYACGT" * 5, "ACGTRYACGT" * 5),
    ]


def test_aligner_degenerate_and_non_acgt(racon):
    """§1e + §1f. Empty sequences return ("", -1, 2). Equal non-ACGT bytes
    match on the CPU aligner (Peq::code_of) but not in the kernel's
    base_code, so such pairs must either fall back (status != 0) or report
    the byte-equality distance (the host refuses pairs with such bytes on
    both sides; with them on one side only the two rules agree). Regression: ("ACGTNNNNACGT", same) used to
    come back status 0 with distance 4. Neighbouring ordinary pairs must be
    unaffected by either kind of skipped pair."""
    rng = random.Random(5001)
    normal = []
    for n in (5, 64, 200, 700):
        t = _rand_seq(rng, n)
        normal.append((_mutate(rng, t, 0.01, 0.01, 0.01) or "A", t))
    degenerate = [("", "ACG"), ("ACG", ""), ("", "")]
    nonacgt = [(q, t) for _, q, t in nonacgt_pairs()]

    batch = [normal[0], degenerate[0], nonacgt[0], normal[1], degenerate[1]]
    batch += nonacgt[1:5] + [normal[2], degenerate[2]] + nonacgt[5:] + [normal[3]]
    res = dict(zip(range(len(batch)), racon.gpu_align(batch)))
    alone = racon.gpu_align(normal)

    by_pair = {}
    for k, p in enumerate(batch):
        by_pair.setdefault(p, res[k])
    for p in degenerate:
        assert by_pair[p] == ("", -1, 2), (p, by_pair[p])
    for p, r in zip(normal, alone):
        assert_exact(racon, "normal", p[0], p[1], r, np_edit_distance(*p))
        assert by_pair[p] == r, "neighbour of a skipped pair changed"
    for (tag, q, t) in nonacgt_pairs():
        cigar, ed, status = by_pair[(q, t)]
        if status != 0:
            assert cigar == "", tag
            continue
        want = racon.edit_distance(q, t)
        assert want == np_edit_distance(q, t)
        assert ed == want, (tag, ed, want)


# --------------------------------------------------------------------------
# 2. POA differ
# --------------------------------------------------------------------------

def _window(bb, layers, bbq=None):
    """Window in differ form; layer spans use the pipeline's inclusive end."""
    blen = len(bb)
    out = [(bb, bbq if bbq is not None else "!" * blen, 0, 0)]
    for item in layers:
        seq, qual = item if isinstance(item, tuple) else (item, "")
        out.append((seq[:1023], qual[:1023], 0, blen - 1))
    return out


def _mutated_window(rng, blen, depth, err=(0.02, 0.02, 0.02)):
    bb = _rand_seq(rng, blen)
    return _window(bb, [_mutate(rng, bb, *err) for _ in range(depth)])


def _sub_only_window(rng, blen, depth, rate):
    bb = _rand_seq(rng, blen)
    return _window(bb, [_mutate(rng, bb, rate, 0.0, 0.0) for _ in range(depth)])


def _with_inserts(rng, seq, count):
    out = list(seq)
    for pos in sorted(rng.sample(range(1, len(seq)), count), reverse=True):
        out.insert(pos, rng.choice("ACGT"))
    return "".join(out)


def bucket_boundary_windows():
    """§2a: (tag, window). Tier T0."""
    rng = random.Random(6000)
    wins = []
    for blen in (319, 320, 321, 574, 575, 576, 577):
        wins.append((f"2a mut blen={blen}", _mutated_window(rng, blen, 12)))
        # substitution-only layers pin max_len to exactly blen
        wins.append((f"2a exact max_len={blen}", _sub_only_window(rng, blen, 12, 0.04)))
    for blen, extra in ((300, 25), (560, 20)):
        # one insert-heavy layer decides max_len (325 > 320, 580 > 575)
        bb = _rand_seq(rng, blen)
        layers = [_mutate(rng, bb, 0.03, 0.0, 0.0) for _ in range(11)]
        layers.insert(5, _with_inserts(rng, bb, extra))
        wins.append((f"2a long layer blen={blen}", _window(bb, layers)))
    for depth in (94, 95, 96):
        # num_seqs 95 / 96 / 97 around the <= 96 route. 2% error in all keeps
        # the graph (~1200 nodes) under the 1535-node cap of the variant that
        # num_seqs <= 96 selects; at 2% each of sub/ins/del the same window
        # grows to ~1800 nodes and fails over by design (see
        # test_poa_node_overflow_fails_over).
        wins.append((f"2a depth={depth}", _mutated_window(rng, 500, depth,
                                                          (0.01, 0.005, 0.005))))
    return wins


SHORT_LENGTHS = (1, 2, 3, 37, 63, 64, 65, 99, 100, 101)


def short_windows():
    """§2b: (tag, tier, window); tier "eq" = bit-equal, "t1" = T1."""
    rng = random.Random(6100)
    wins = []
    for blen in SHORT_LENGTHS:
        wins.append((f"2b sub-only blen={blen}", "eq", _sub_only_window(rng, blen, 6, 0.05)))
    for blen in SHORT_LENGTHS:
        bb = _rand_seq(rng, blen)
        layers = [_mutate(rng, bb, 0.01, 0.01, 0.01) or bb[0] for _ in range(6)]
        wins.append((f"2b indel blen={blen}", "t1", _window(bb, layers)))
    for blen in (37, 64):
        bb = _rand_seq(rng, blen)
        layers = [_mutate(rng, bb, 0.01, 0.01, 0.01) for _ in range(6)]
        layers[2:2] = [bb[blen // 2], bb[5:7]]  # a 1-base and a 2-base layer
        wins.append((f"2b tiny layers blen={blen}", "t1", _window(bb, layers)))
    return wins


def _with_n_runs(seq):
    s = list(seq)
    for at, run in ((40, 1), (90, 5), (150, 70)):
        s[at:at + run] = "N" * run
    return "".join(s)


def non_acgt_windows():
    """§2d non-ACGT: N runs of 1, 5 and 70 in the backbone, in layers, and in
    both at the same place. Tier T0."""
    rng = random.Random(6200)
    wins = []
    for blen in (300, 700):
        bb = _rand_seq(rng, blen)
        clean = [_mutate(rng, bb, 0.02, 0.02, 0.02) for _ in range(10)]
        wins.append((f"2d N backbone blen={blen}", _window(_with_n_runs(bb), clean)))
        half = [_with_n_runs(_mutate(rng, bb, 0.02, 0.0, 0.0)) if k % 2 else s
                for k, s in enumerate(clean)]
        wins.append((f"2d N layers blen={blen}", _window(bb, half)))
        nbb = _with_n_runs(bb)
        both = [_mutate(rng, nbb, 0.02, 0.02, 0.02) for _ in range(10)]
        wins.append((f"2d N both blen={blen}", _window(nbb, both)))
    return wins


def quality_windows():
    """§2d quality: per-layer quality strings — all '!' (weight 0), all '~'
    (weight 93), random, and none — over a backbone with random qualities."""
    rng = random.Random(6300)
    wins = []
    for blen in (310, 500):
        bb = _rand_seq(rng, blen)
        bbq = "".join(chr(33 + rng.randrange(94)) for _ in range(blen))
        layers = []
        for k in range(16):
            s = _mutate(rng, bb, 0.02, 0.02, 0.02)
            q = ("", "!" * len(s), "~" * len(s),
                 "".join(chr(33 + rng.randrange(94)) for _ in range(len(s))))[k % 4]
            layers.append((s, q))
        wins.append((f"2d quality blen={blen}", _window(bb, layers, bbq)))
    return wins


def assert_t0(tag, cpu, gpu):
    assert gpu[1], f"{tag}: GPU window failed over to the CPU"
    assert cpu[1], tag
    assert gpu[0] == cpu[0], (tag, len(cpu[0]), len(gpu[0]))


def assert_t1(racon, tag, cpu, gpu):
    assert gpu[1], f"{tag}: GPU window failed over to the CPU"
    ed = racon.edit_distance(cpu[0], gpu[0])
    assert ed <= max(4, len(cpu[0]) // 100), (tag, ed, cpu[0], gpu[0])


@pytest.fixture(scope="module")
def main_batch(racon):
    """One CPU and one GPU run over the §2a, §2b and default-parameter §2d
    windows; shared by the tier tests and the batch-composition test."""
    rng = random.Random(6400)
    cases = [(tag, "t0", w) for tag, w in bucket_boundary_windows()]
    cases += short_windows()
    cases += [(tag, "t0", w) for tag, w in non_acgt_windows() + quality_windows()]
    # twins with identical total layer bytes: equal-cost ties in the sort
    for blen in (320, 575, 37):
        cases.append((f"2f tie twin blen={blen}", "eq", _sub_only_window(rng, blen, 12, 0.04)))
        cases.append((f"2f tie twin' blen={blen}", "eq", _sub_only_window(rng, blen, 12, 0.04)))
    windows = [w for _, _, w in cases]
    cpu = racon.poa_windows_cpu(windows)
    gpu = racon.poa_windows_gpu(windows)
    return cases, cpu, gpu


def _check_tiers(racon, main_batch, prefix):
    cases, cpu, gpu = main_batch
    seen = 0
    for (tag, tier, w), c, g in zip(cases, cpu, gpu):
        if not tag.startswith(prefix):
            continue
        seen += 1
        if len(w[0][0]) == 1:
            # a 1-base backbone cannot take layers (the inclusive span 0..0 is
            # empty for add_layer): both engines pass the backbone through
            assert c == (w[0][0], False) and g == c, (tag, c, g)
        elif tier == "t0":
            assert_t0(tag, c, g)
        elif tier == "eq":
            assert g[1], f"{tag}: GPU window failed over to the CPU"
            assert g[0] == c[0], (tag, c[0], g[0])
        else:
            assert_t1(racon, tag, c, g)
    assert seen > 0


def test_poa_bucket_boundaries(racon, main_batch):
    """§2a: lengths, one long layer, and depths around every routing threshold
    of PoaBatch::generate are bit-equal to the CPU engine (a mis-route ends
    in kPoaWidthOverflow, i.e. ok == False)."""
    deep = [w for tag, w in bucket_boundary_windows() if tag.startswith("2a depth")]
    # test-input sanity: under the smallest node cap either route can meet
    assert max(racon.poa_window_node_counts(deep)) <= 1400
    _check_tiers(racon, main_batch, "2a")


def test_poa_short_trailing_windows(racon, main_batch):
    """§2b: windows shorter than every margin (edge_margin == 0 below 100 bp,
    so every layer takes the subgraph path on both engines)."""
    _check_tiers(racon, main_batch, "2b")


def test_poa_non_acgt_and_quality_default_params(racon, main_batch):
    """§2d at the default trim/tgs/scores: the non-ACGT row-letter fallback
    in the DP and per-layer quality weights 0..93."""
    _check_tiers(racon, main_batch, "2d")


@pytest.mark.parametrize("trim,tgs", [(False, True), (True, False), (False, False)])
def test_poa_quality_trim_and_tgs(racon, trim, tgs):
    """§2d: quality-weighted and non-ACGT windows under the other trim / tgs
    combinations (the default pair runs in main_batch)."""
    cases = quality_windows() + non_acgt_windows()
    windows = [w for _, w in cases]
    cpu = racon.poa_windows_cpu(windows, trim=trim, tgs=tgs)
    gpu = racon.poa_windows_gpu(windows, trim=trim, tgs=tgs)
    for (tag, _), c, g in zip(cases, cpu, gpu):
        assert_t0(f"{tag} trim={trim} tgs={tgs}", c, g)


NODE_CAP = 2047


def score_windows():
    """300 / 575 / 1000 bp windows at depth 30, plus a 1000 bp window at 6%
    error whose graph approaches the node cap. Depth 30 at 6% would exceed the
    cap (CPU graph ~2190 nodes; test_poa_node_overflow_fails_over covers
    that), so the last window stops at depth 20 (~1900 nodes)."""
    rng = random.Random(6500)
    return [("2d scores blen=300", _mutated_window(rng, 300, 30)),
            ("2d scores blen=575", _mutated_window(rng, 575, 30)),
            ("2d scores blen=1000", _mutated_window(rng, 1000, 30, (0.01, 0.005, 0.005))),
            ("2d scores blen=1000 6%", _mutated_window(rng, 1000, 20))]


@pytest.mark.parametrize("scores", [(1, -1, -1), (5, -4, -8), (8, -6, -8), (9, -9, -9)])
def test_poa_score_sets(racon, scores):
    """§2d: score sets up to the |param| <= 9 int16 guard. Tier T0."""
    m, x, g = scores
    cases = score_windows()
    windows = [w for _, w in cases]
    counts = racon.poa_window_node_counts(windows, match=m, mismatch=x, gap=g)
    # test-input sanity: nothing overflows, the last window comes close
    assert max(counts) <= 2000 < NODE_CAP and counts[-1] >= 1800, counts
    cpu = racon.poa_windows_cpu(windows, match=m, mismatch=x, gap=g)
    gpu = racon.poa_windows_gpu(windows, match=m, mismatch=x, gap=g)
    for (tag, _), c, gg in zip(cases, cpu, gpu):
        assert_t0(f"{tag} scores={scores}", c, gg)


def test_poa_score_guard_refuses_10(racon):
    """(10,-10,-10) exceeds the int16 score guard: the PoaBatch constructor
    throws before anything runs."""
    rng = random.Random(6501)
    with pytest.raises(RuntimeError, match="score parameters too large"):
        racon.poa_windows_gpu([_mutated_window(rng, 200, 4)], match=10, mismatch=-10, gap=-10)


def test_poa_capacity_layers_depth_backbone(racon):
    """§2c: over-long layers and layers past depth 200 are dropped; a 1023-base
    backbone runs and a 1024-base one is rejected. GPU-vs-GPU, bit-exact."""
    rng = random.Random(6600)

    # over-long layers: 1024, 1100 and 1500 bases are dropped on the device
    base = _mutated_window(rng, 1000, 14)
    bb = base[0][0]
    longs = [(_fit_length(rng, _mutate(rng, bb, 0.02, 0.02, 0.02), n), "", 0, 999)
             for n in (1024, 1100, 1500)]
    with_long = base[:5] + longs[:1] + base[5:9] + longs[1:] + base[9:]

    # depth cap: layers k = 0..209 with distinct begins; the last 10 carry a
    # foreign 20-base insert at weight 93 that would win if it were shipped
    dbb = _rand_seq(rng, 1000)
    insert = "ACGTTGCA" + "GGATCCATGCAT"
    deep = [(dbb, "!" * 1000, 0, 0)]
    for k in range(210):
        seg = dbb[k:]
        if k < 200:
            deep.append((_mutate(rng, seg, 0.002, 0.0, 0.0), "", k, 999))
        else:
            s = seg[:600 - k] + insert + seg[600 - k:]
            deep.append((s, "~" * len(s), k, 999))
    assert insert not in dbb
    # the 200 shipped layers must fit the device graph (node cap 2047)
    assert racon.poa_window_node_counts([deep[:201]])[0] <= 1600
    cpu_deep = racon.poa_windows_cpu([deep])[0]
    assert insert in cpu_deep[0], "test input must make the insert win when all layers count"

    w1023 = _sub_only_window(rng, 1023, 6, 0.02)
    w1024 = _sub_only_window(rng, 1024, 6, 0.02)
    assert len(w1023[0][0]) == 1023 and len(w1024[0][0]) == 1024

    gpu = racon.poa_windows_gpu([with_long, base, deep, deep[:201], w1023, w1024])
    cpu_base = racon.poa_windows_cpu([base])[0]
    assert gpu[0] == gpu[1], "over-long layers changed the window's result"
    assert_t0("2c over-long layers dropped", cpu_base, gpu[0])
    assert gpu[2][1] and gpu[3][1], (gpu[2][1], gpu[3][1])
    assert gpu[2] == gpu[3], "layers past depth 200 were not dropped"
    assert insert not in gpu[2][0]
    assert gpu[4][1] and len(gpu[4][0]) > 900, gpu[4][1]
    assert gpu[5] == ("", False)


def node_overflow_windows():
    """§2c: insert-heavy windows whose CPU graphs exceed the node caps:
    [0] 1000 bp, >= 2300 nodes (cap 2047); [1] 500 bp, <= 96 sequences,
    rows <= 575 columns, >= 1800 nodes (bucket 1's cap is 1535)."""
    rng = random.Random(6700)
    big = _mutated_window(rng, 1000, 30, (0.05, 0.10, 0.10))
    small = _mutated_window(rng, 500, 30, (0.05, 0.10, 0.10))
    return [big, small]


def test_poa_node_overflow_fails_over(racon):
    """§2c: a window that outgrows the node cap reports ok == False (the
    kPoaNodeOverflow path) and leaves every other window of the call alone."""
    rng = random.Random(6701)
    over = node_overflow_windows()
    counts = racon.poa_window_node_counts(over)
    # [1] sits between bucket 1's 1535-node cap and the full 2047 cap, so it
    # fails over only if the smaller variant enforces its own cap
    assert counts[0] >= 2300 and 1800 <= counts[1] < NODE_CAP, counts
    assert len(over[1]) <= 96 and max(len(l[0]) for l in over[1]) <= 575

    others = [_mutated_window(rng, 500, 20), _mutated_window(rng, 1000, 12),
              _mutated_window(rng, 300, 8), _mutated_window(rng, 520, 30)]
    mixed = [others[0], over[0], others[1], others[2], over[1], others[3]]
    got = racon.poa_windows_gpu(mixed)
    alone = racon.poa_windows_gpu(others)
    for k in (1, 4):
        if got[k][1]:  # report instead of only failing: compare with the CPU
            cpu = racon.poa_windows_cpu([mixed[k]])[0]
            print(f"overflow window {k} returned ok with ed "
                  f"{racon.edit_distance(cpu[0], got[k][0])} to the CPU consensus")
        assert got[k][1] is False, f"window {k} ({counts}) did not fail over"
    assert [got[0], got[2], got[3], got[5]] == alone
    assert all(ok for _, ok in alone)


BANDED_LENGTHS = (255, 256, 257, 300, 320, 321, 575, 576, 700, 1000)


def test_poa_banded_boundaries(racon):
    """§2e: the bw < len threshold (255/256/257) and banded windows in every
    banded route (bucket 0 above 256 columns, 3, and 4). Tier T2."""
    rng = random.Random(6800)
    windows = [_mutated_window(rng, blen, 24) for blen in BANDED_LENGTHS]
    cpu = racon.poa_windows_cpu(windows)
    gpu = racon.poa_windows_gpu(windows, banded=True)
    excluded = [blen for blen, g in zip(BANDED_LENGTHS, gpu) if not g[1]]
    assert len(excluded) <= 1, excluded
    for blen, c, g in zip(BANDED_LENGTHS, cpu, gpu):
        if g[1]:
            ed = racon.edit_distance(c[0], g[0])
            print(f"banded blen={blen}: ed {ed}")
            assert ed <= 2, (blen, ed)


def test_poa_batch_composition(racon, main_batch):
    """§2f: a batch mixing every non-banded kernel variant, with equal-cost
    ties, gives each window the same (consensus, ok) in any order and alone."""
    cases, _, gpu = main_batch
    windows = [w for _, _, w in cases]
    n = len(windows)

    rev = racon.poa_windows_gpu(windows[::-1])[::-1]
    assert rev == gpu, [cases[k][0] for k in range(n) if rev[k] != gpu[k]]

    perm = list(range(n))
    random.Random(6900).shuffle(perm)
    shuf = racon.poa_windows_gpu([windows[k] for k in perm])
    bad = [cases[k][0] for j, k in enumerate(perm) if shuf[j] != gpu[k]]
    assert bad == []

    pick = [k for k, (tag, _, _) in enumerate(cases)
            if tag in ("2a exact max_len=320", "2a exact max_len=321", "2a mut blen=576",
                       "2a depth=96", "2b indel blen=37", "2f tie twin' blen=575")]
    assert len(pick) == 6
    alone = racon.poa_windows_gpu([windows[k] for k in pick])
    assert alone == [gpu[k] for k in pick]


_TIMED_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import _racon
plain, banded = json.load(open(sys.argv[2]))
as_windows = lambda ws: [[tuple(layer) for layer in w] for w in ws]
print(json.dumps([_racon.poa_windows_gpu(as_windows(plain)),
                  _racon.poa_windows_gpu(as_windows(banded), banded=True)]))
"""


def test_poa_timed_instantiations(racon, tmp_path):
    """RGA_POA_TIMING selects the five TIMED=true kernel instantiations, which
    nothing else launches. One window per variant (narrow, mid, full by depth,
    banded mid, banded full) in a fresh process with the variable set must
    give exactly what this process gives without it, with every window ok."""
    import json
    import os
    import subprocess
    import sys

    assert "RGA_POA_TIMING" not in os.environ  # read once per process
    rng = random.Random(7000)
    plain = [_mutated_window(rng, 300, 12), _mutated_window(rng, 500, 12),
             _mutated_window(rng, 500, 96, (0.01, 0.005, 0.005))]
    banded = [_mutated_window(rng, 500, 12), _mutated_window(rng, 700, 12)]
    # test-input sanity: the windows land where the routing thresholds say
    longest = [max(len(layer[0]) for layer in w) for w in plain + banded]
    assert longest[0] <= 320 and all(321 <= n <= 575 for n in longest[1:4]) and longest[4] >= 576
    assert len(plain[2]) == 97

    want = [racon.poa_windows_gpu(plain), racon.poa_windows_gpu(banded, banded=True)]
    args = tmp_path / "windows.json"
    args.write_text(json.dumps([plain, banded]))
    child = subprocess.run(
        [sys.executable, "-c", _TIMED_CHILD, os.path.dirname(racon.__file__), str(args)],
        env=dict(os.environ, RGA_POA_TIMING="1"), capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    got = [[tuple(r) for r in call] for call in json.loads(child.stdout)]
    assert got == want
    assert all(ok for call in got for _, ok in call), got
    assert child.stderr.count("timing (wall ticks") == 2, child.stderr[-2000:]


def test_pipeline_n_in_draft_and_reads(racon, sample, fasta_reader, tmp_path):
    """Drafts with N runs are ordinary input. Here the draft has a 30-base N
    run and every read carries an N, so Sequence::acgt_only is false on both
    sides of every overlap: add_overlap scans the spans, the overlaps that
    hold non-ACGT bytes on both sides go to the CPU aligner, and the polish
    still repairs the draft, independent of the batch layout."""
    truth = list(fasta_reader(sample["reference"]).values())[0]
    name, draft = list(fasta_reader(sample["layout"]).items())[0]
    draft = draft[:10000] + "N" * 30 + draft[10030:]
    layout = tmp_path / "layout_n.fasta"
    layout.write_text(f">{name}\n{draft}\n")
    reads = tmp_path / "reads_n.fasta"
    with open(reads, "w") as f:
        for rname, seq in fasta_reader(sample["reads"]).items():
            at = len(seq) // 2
            f.write(f">{rname}\n{seq[:at]}N{seq[at + 1:]}\n")
    before = racon.edit_distance(draft, truth)

    a = racon.polish(str(reads), sample["overlaps"], str(layout),
                     threads=4, poa_batches=1, aligner_batches=1)
    b = racon.polish(str(reads), sample["overlaps"], str(layout),
                     threads=2, poa_batches=2, aligner_batches=2)
    assert a == b
    assert len(a) == 1 and "N" not in a[0][1]
    assert racon.edit_distance(a[0][1], truth) < before * 0.2
