"""The HIP aligner's adaptive band (band_policy="adaptive" / "retry").

The specification is tools/sim_myers.py's align(..., adaptive=True): the
kernel runs the same recurrence with the same band rule, so status, distance
and CIGAR must be equal to the simulator's, not close. Independent checks on
top of that: np_edit_distance for the optimum, replay_cigar for the cost of
the CIGAR, breaking_points_from_cigar for the breaking-point traceback.

The pinned inputs are built here and imported by test_adaptive_band_sim.py,
which holds them (on the CPU, with the simulator) to the conditions that make
them worth running: every "rescued" pair escapes the diagonal band and is
completed optimally by the adaptive one, every "limit" pair is beyond it.
"""

import itertools
import json
import os
import random
import subprocess
import sys
from pathlib import Path

import pytest

from test_gpu_kernel_edges import (_fit_length, _mutate, _rand_seq, np_edit_distance,
                                   replay_cigar)

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import sim_myers  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def require_gpu(racon):
    # torch is deliberately not imported (see test_gpu_kernel_edges.py)
    if racon.device_count() < 1:
        pytest.skip("no GPU on this host")


# --------------------------------------------------------------------------
# input builders (deterministic; shared with test_adaptive_band_sim.py)
# --------------------------------------------------------------------------

def _noisy(rng, seq, rate=0.02):
    """seq with substitutions only, so the lengths stay what the case names."""
    return _mutate(rng, seq, rate, 0.0, 0.0)


def query_blocks_pair(rng, m, L):
    """Target of m bases; the query is the target at 2 % substitutions plus
    three random L-base blocks the target lacks, at 20 / 40 / 60 % of it."""
    t = _rand_seq(rng, m)
    q = _noisy(rng, t)
    for frac in (0.6, 0.4, 0.2):  # back to front: positions stay valid
        at = int(m * frac)
        q = q[:at] + _rand_seq(rng, L) + q[at:]
    return q, t


def target_blocks_pair(rng, m, L):
    """Target of m bases; the query is the target at 2 % substitutions minus
    the three L-base blocks at 20 / 40 / 60 % of the target."""
    t = _rand_seq(rng, m)
    q = _noisy(rng, t)
    for frac in (0.6, 0.4, 0.2):
        at = int(m * frac)
        q = q[:at] + q[at + L:]
    return q, t


def query_end_pair(rng, m, delta):
    """delta < 0: the query lacks the target's last -delta bases; delta > 0:
    it carries delta extra bases after the target's end."""
    t = _rand_seq(rng, m)
    q = _noisy(rng, t)
    q = q[:delta] if delta < 0 else q + _rand_seq(rng, delta)
    return q, t


def target_block_at_pair(rng, m, L, at):
    """One L-base block of the target, at position `at`, that the query lacks."""
    t = _rand_seq(rng, m)
    q = _noisy(rng, t)
    return q[:at] + q[at + L:], t


def rescued_pairs():
    """(tag, band, query, target): the diagonal band escapes, the adaptive
    band completes with the optimal distance."""
    return [
        ("3x60 query-only blocks", 256, *query_blocks_pair(random.Random(9101), 2000, 60)),
        ("3x90 query-only blocks", 256, *query_blocks_pair(random.Random(9102), 2000, 90)),
        ("300 missing at the query's end", 256, *query_end_pair(random.Random(9103), 1500, -300)),
        ("3x180 query-only blocks, K=8", 512, *query_blocks_pair(random.Random(9105), 4000, 180)),
    ]


def limit_pairs():
    """(tag, band, query, target) beyond what the adaptive band follows: it
    escapes or returns a distance above the optimum."""
    return [
        ("200-base target-only block at 200", 256,
         *target_block_at_pair(random.Random(9101), 2000, 200, 200)),
        ("3x90 target-only blocks", 256, *target_blocks_pair(random.Random(9102), 2000, 90)),
        ("3x120 query-only blocks", 256, *query_blocks_pair(random.Random(9103), 2000, 120)),
    ]


SAME_N = (1, 63, 64, 65, 255, 256)  # n <= 64 * K at K = 4: the band cannot move
SLIDE_N = (257, 320, 384)           # hi = 1 (first possible slide), and 64 * (K + 2)


def _length_grid(ns, seed):
    rng = random.Random(seed)
    pairs = []
    for n in ns:
        q = _rand_seq(rng, n)
        for m in (max(1, n // 2), n, 2 * n):
            t = _fit_length(rng, _mutate(rng, q, 0.01, 0.01, 0.01), m)
            pairs.append((f"n={n} m={m}", 256, q, t))
    return pairs


def same_pairs():
    """(tag, band, query, target) whose query fits the K = 4 band."""
    return _length_grid(SAME_N, 9301)


def slide_pairs():
    """The shortest queries whose band can move; m = n/2 forces the slides."""
    return _length_grid(SLIDE_N, 9302)


def noise_pairs():
    """About 60 pairs at 2 % noise, lengths 3..1500 interleaved so that every
    16-lane wave mixes short and long lanes."""
    rng = random.Random(9401)
    pairs = []
    for k in range(60):
        t_len = 3 + (k * 577) % 1498
        t = _rand_seq(rng, t_len)
        q = _mutate(rng, t, 0.01, 0.005, 0.005) or rng.choice("ACGT")
        pairs.append((f"noise {k} t_len={t_len}", 256, q, t))
    return pairs


def mixed_pairs():
    """One K = 4 call's worth: same, slide, rescued and limit pairs spread
    among the noise pairs (about 80 in all, several 16-lane waves)."""
    special = [p for p in same_pairs()[::3] + slide_pairs()[::4] + rescued_pairs() + limit_pairs()
               if p[1] == 256]
    noise = noise_pairs()
    out = []
    step = len(noise) // len(special)
    for k, p in enumerate(special):
        out.extend(noise[k * step:(k + 1) * step])
        out.append(p)
    out.extend(noise[len(special) * step:])
    return out


def n_in_query_pair():
    """A rescued pair with one N in the query only (the target stays pure
    A/C/G/T, so the device and the CPU aligner agree on what N costs)."""
    tag, band, q, t = rescued_pairs()[0]
    at = len(q) // 2
    return tag + ", N in the query", band, q[:at] + "N" + q[at + 1:], t


# --------------------------------------------------------------------------
# simulator as oracle
# --------------------------------------------------------------------------

def cigar_of_path(path):
    return "".join(f"{len(list(g))}{op}" for op, g in itertools.groupby(path))


_SIM_CACHE = {}


def sim_result(q, t, band, adaptive):
    """The simulator's answer in gpu_align's terms: (cigar, distance, status).
    An escape found at the final cell has no distance (-1); one found during
    the traceback keeps the forward pass's."""
    key = (q, t, band, adaptive)
    if key not in _SIM_CACHE:
        ed, path, st = sim_myers.align(q, t, band // 64, adaptive=adaptive)
        if st == "ok":
            _SIM_CACHE[key] = (cigar_of_path(path), ed, 0)
        else:
            _SIM_CACHE[key] = ("", -1 if ed is None else ed, 1)
    return _SIM_CACHE[key]


_OPT_CACHE = {}


def optimum(q, t):
    if (q, t) not in _OPT_CACHE:
        _OPT_CACHE[(q, t)] = np_edit_distance(q, t)
    return _OPT_CACHE[(q, t)]


def gpu_align(racon, cases, policy):
    """cases share one band; returns gpu_align's tuples."""
    bands = {c[1] for c in cases}
    assert len(bands) == 1
    return racon.gpu_align([(q, t) for _, _, q, t in cases], band_width=bands.pop(),
                           band_policy=policy)


def by_band(cases):
    return [[c for c in cases if c[1] == band] for band in sorted({c[1] for c in cases})]


# --------------------------------------------------------------------------
# tests
# --------------------------------------------------------------------------

def test_same(racon):
    """A query of at most 64 * K rows never moves the band: adaptive equals
    diagonal. From n = 257 on it can move, and equals the simulator."""
    cases = same_pairs()
    diagonal = gpu_align(racon, cases, "diagonal")
    adaptive = gpu_align(racon, cases, "adaptive")
    for (tag, *_), d, a in zip(cases, diagonal, adaptive):
        assert a == d, tag
    assert all(status == 0 for _, _, status in diagonal)

    cases = slide_pairs()
    for (tag, band, q, t), got in zip(cases, gpu_align(racon, cases, "adaptive")):
        assert got == sim_result(q, t, band, True), tag


def test_rescued(racon):
    for cases in by_band(rescued_pairs()):
        diagonal = gpu_align(racon, cases, "diagonal")
        adaptive = gpu_align(racon, cases, "adaptive")
        for (tag, band, q, t), d, a in zip(cases, diagonal, adaptive):
            assert d[2] != 0 and d[0] == "", (tag, d[1:])
            cigar, ed, status = a
            print(f"{tag}: diagonal status {d[2]}, adaptive status {status} distance {ed}, "
                  f"optimum {optimum(q, t)}")
            assert status == 0, tag
            assert ed == optimum(q, t), tag
            assert replay_cigar(q, t, cigar) == (len(q), len(t), ed), tag
            assert cigar == sim_result(q, t, band, True)[0], tag


def test_limit(racon):
    cases = limit_pairs()
    for (tag, band, q, t), got in zip(cases, gpu_align(racon, cases, "adaptive")):
        assert got == sim_result(q, t, band, True), tag
        cigar, ed, status = got
        print(f"{tag}: adaptive status {status} distance {ed}, optimum {optimum(q, t)}")
        if status == 0:
            assert replay_cigar(q, t, cigar) == (len(q), len(t), ed), tag
            assert ed >= optimum(q, t), tag
        else:
            assert cigar == "", tag


_RETRY_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import _racon
pairs = [tuple(p) for p in json.load(open(sys.argv[2]))]
print(json.dumps([_racon.gpu_align(pairs, band_width=256, band_policy=p)
                  for p in ("diagonal", "adaptive", "retry")]))
"""


def assert_retry_contract(cases, diagonal, adaptive, retry):
    retried = 0
    for (tag, *_), d, a, r in zip(cases, diagonal, adaptive, retry):
        if d[2] == 0:
            assert r == d, tag
        else:
            assert r == a, tag
            retried += 1
    return retried


def test_retry(racon, tmp_path):
    """retry = diagonal, then adaptive over the escaped alignments only."""
    assert "RGA_ALN_LANES" not in os.environ
    cases = mixed_pairs()
    assert 75 <= len(cases) <= 90
    diagonal, adaptive, retry = (gpu_align(racon, cases, p)
                                 for p in ("diagonal", "adaptive", "retry"))
    retried = assert_retry_contract(cases, diagonal, adaptive, retry)
    completed = sum(1 for d, r in zip(diagonal, retry) if d[2] != 0 and r[2] == 0)
    print(f"{len(cases)} pairs: {retried} escaped the diagonal band, "
          f"{completed} completed by the second pass")
    # test-input sanity: the second pass had work, finished some of it and
    # left some escaped
    assert 0 < completed < retried

    args = tmp_path / "pairs.json"
    args.write_text(json.dumps([(q, t) for _, _, q, t in cases]))
    child = subprocess.run(
        [sys.executable, "-c", _RETRY_CHILD, os.path.dirname(racon.__file__), str(args)],
        env=dict(os.environ, RGA_ALN_LANES="64"), capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    packed = [[tuple(r) for r in results] for results in json.loads(child.stdout)]
    assert packed == [diagonal, adaptive, retry]


@pytest.mark.parametrize("window_length", [64, 500])
@pytest.mark.parametrize("policy", ["adaptive", "retry"])
def test_breaking_points(racon, policy, window_length):
    """The breaking-point traceback reads the same recorded band tops: its
    points equal the CIGAR walk over the path traceback's result."""
    for cases in by_band(rescued_pairs()) + [mixed_pairs()]:
        pairs = [(q, t) for _, _, q, t in cases]
        band = cases[0][1]
        t_begins = [(k * 137) % 1000 + 1 for k in range(len(cases))]
        q_begins = [(k * 29) % 200 + 1 for k in range(len(cases))]
        paths = racon.gpu_align(pairs, band_width=band, band_policy=policy)
        got = racon.gpu_breaking_points(pairs, window_length, t_begins=t_begins,
                                        q_begins=q_begins, band_width=band,
                                        band_policy=policy)
        assert len(got) == len(cases)
        escaped = 0
        for (tag, _, q, t), (cigar, ed, status), tb, qb, g in zip(
                cases, paths, t_begins, q_begins, got):
            want = []
            if status == 0:
                want = racon.breaking_points_from_cigar(cigar, window_length, tb, tb + len(t), qb)
            else:
                escaped += 1
            assert g == (want, ed, status), tag
        if len(cases) > 10:
            assert escaped > 0, "test input: no pair of the mixed set stayed escaped"


def test_non_acgt(racon):
    tag, band, q, t = n_in_query_pair()
    got = racon.gpu_align([(q, t)], band_width=band, band_policy="adaptive")[0]
    assert got == sim_result(q, t, band, True), tag
    assert got[2] == 0 and got[1] == optimum(q, t), tag


# --------------------------------------------------------------------------
# pipeline
# --------------------------------------------------------------------------

def pipeline_sample(d):
    """One 6 kbp contig (the truth at 1 % substitutions and small indels), 12
    full-length reads at 2 % noise, 4 of them with three extra 90-base
    blocks, and a PAF that maps every read onto the whole contig."""
    rng = random.Random(9501)
    truth = _rand_seq(rng, 6000)
    draft = _mutate(rng, truth, 0.01, 0.005, 0.005)
    reads = []
    for k in range(12):
        read = _mutate(rng, truth, 0.01, 0.005, 0.005)
        if k % 3 == 0:
            for frac in (0.6, 0.4, 0.2):
                at = int(len(read) * frac)
                read = read[:at] + _rand_seq(rng, 90) + read[at:]
        reads.append(read)
    d = Path(d)
    (d / "draft.fasta").write_text(f">contig\n{draft}\n")
    (d / "reads.fasta").write_text("".join(f">read{k}\n{r}\n" for k, r in enumerate(reads)))
    (d / "overlaps.paf").write_text("".join(
        f"read{k}\t{len(r)}\t0\t{len(r)}\t+\tcontig\t{len(draft)}\t0\t{len(draft)}\t"
        f"{min(len(r), len(draft))}\t{max(len(r), len(draft))}\t255\n"
        for k, r in enumerate(reads)))
    return dict(reads=str(d / "reads.fasta"), overlaps=str(d / "overlaps.paf"),
                draft=str(d / "draft.fasta"), truth=truth, draft_seq=draft, read_seqs=reads)


def test_pipeline(racon, racon_cli, fasta_reader, tmp_path):
    s = pipeline_sample(tmp_path)
    base = [racon_cli, "--cudaaligner-batches", "1", "--cudaaligner-band-width", "256",
            "-c", "1", "-t", "4"]
    inputs = [s["reads"], s["overlaps"], s["draft"]]

    def run(cmd):
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=tmp_path)
        assert p.returncode == 0, p.stderr[-2000:]
        return p

    plain = run(base + inputs)
    assert "4 overlap(s) aligned on CPU" in plain.stderr, plain.stderr[-2000:]
    assert "completed by the adaptive band" not in plain.stderr

    first = run(base + ["--aligner-adaptive-band"] + inputs)
    second = run(base + ["--aligner-adaptive-band"] + inputs)
    assert "aligned on CPU" not in first.stderr, first.stderr[-2000:]
    assert "4 overlap(s) completed by the adaptive band" in first.stderr, first.stderr[-2000:]
    assert first.stdout and first.stdout == second.stdout

    (tmp_path / "polished.fasta").write_text(first.stdout)
    polished = fasta_reader(tmp_path / "polished.fasta")
    assert len(polished) == 1
    before = racon.edit_distance(s["draft_seq"], s["truth"])
    after = racon.edit_distance(next(iter(polished.values())), s["truth"])
    print(f"edit distance to the truth: draft {before}, polished {after}")
    assert after < before

    wrapper = Path(__file__).resolve().parent.parent / "scripts" / "racon_wrapper.py"
    wrapped = run([sys.executable, str(wrapper), "--in-process", "--cudaaligner-batches", "1",
                   "--cudaaligner-band-width", "256", "-c", "1", "-t", "4",
                   "-m", "3", "-x", "-5", "-g", "-4", "--aligner-adaptive-band"] + inputs)
    assert "4 overlap(s) completed by the adaptive band" in wrapped.stderr, wrapped.stderr[-2000:]
    assert wrapped.stdout == first.stdout

    with pytest.raises(ValueError):
        racon.gpu_align([("ACGT", "ACGT")], band_policy="bogus")
