"""The HIP aligner's wide band: one wavefront per alignment, 64 blocks of 64
rows (band_policy="wide", wide_pass=True, --aligner-wide-band).

The specification is tools/sim_myers.py's align(q, t, 64), the diagonal band
at K = 64; align_wave() there models the kernel's schedule and is held to
align() in test_wide_band_sim.py. The kernel must return the simulator's
status, distance and CIGAR exactly. Independent checks on top of that:
np_edit_distance for the optimum, replay_cigar for the cost of the CIGAR,
breaking_points_from_cigar for the breaking-point traceback.

A pair whose band would slide more than one block per column (a query more
than 64 times its target and longer than the band) is refused by the host and
comes back as an escape; sim_myers.align_wave says "refused" for it.

The pinned inputs are built here and imported by test_wide_band_sim.py, which
holds them (on the CPU) to the conditions that make them worth running.
"""

import json
import os
import random
import subprocess
import sys
from pathlib import Path

import pytest

import test_adaptive_band_gpu as narrow
from test_adaptive_band_gpu import _noisy, cigar_of_path, optimum, sim_myers
from test_gpu_kernel_edges import _fit_length, _mutate, _rand_seq, replay_cigar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def require_gpu(racon):
    # torch is deliberately not imported (see test_gpu_kernel_edges.py)
    if racon.device_count() < 1:
        pytest.skip("no GPU on this host")


# --------------------------------------------------------------------------
# input builders (deterministic; shared with test_wide_band_sim.py)
# --------------------------------------------------------------------------

FITS_N = (1, 63, 64, 65, 4095, 4096)  # n <= 64 * 64: the band cannot move
SLIDE_N = (4097, 4160, 4224)          # the smallest queries that recycle a lane


def _length_grid(ns, seed):
    rng = random.Random(seed)
    pairs = []
    for n in ns:
        q = _rand_seq(rng, n)
        for m in (max(1, n // 2), n, 2 * n):
            t = _fit_length(rng, _mutate(rng, q, 0.01, 0.01, 0.01), m)
            pairs.append((f"n={n} m={m}", q, t))
    return pairs


def fits_pairs():
    """(tag, query, target) whose query fits the band; for n <= 65 all but
    one or two lanes hold empty blocks."""
    return _length_grid(FITS_N, 9701)


def slide_pairs():
    """The shortest queries whose band moves; m = n/2 slides every 32 columns."""
    return _length_grid(SLIDE_N, 9702)


def query_block_pair(seed):
    """4800-base target; the query is the target at 2 % substitutions with
    1200 random bases inserted at 2400."""
    rng = random.Random(seed)
    t = _rand_seq(rng, 4800)
    q = _noisy(rng, t)
    return q[:2400] + _rand_seq(rng, 1200) + q[2400:], t


def pipeline_sample(d):
    """One 6 kbp contig (the truth at 1 % substitutions and small indels) and
    12 full-length reads at 2 % noise. Reads 0 and 6 carry 300 extra random
    bases at 40 % of their length, reads 3 and 9 lack 300 bases at 60 %. The
    PAF maps every read onto the whole contig."""
    rng = random.Random(9801)
    truth = _rand_seq(rng, 6000)
    draft = _mutate(rng, truth, 0.01, 0.005, 0.005)
    reads = []
    for k in range(12):
        read = _mutate(rng, truth, 0.01, 0.005, 0.005)
        if k % 6 == 0:
            at = int(len(read) * 0.4)
            read = read[:at] + _rand_seq(rng, 300) + read[at:]
        elif k % 6 == 3:
            at = int(len(read) * 0.6)
            read = read[:at] + read[at + 300:]
        reads.append(read)
    out = dict(truth=truth, draft_seq=draft, read_seqs=reads)
    if d is not None:
        d = Path(d)
        (d / "draft.fasta").write_text(f">contig\n{draft}\n")
        (d / "reads.fasta").write_text("".join(f">read{k}\n{r}\n" for k, r in enumerate(reads)))
        (d / "overlaps.paf").write_text("".join(
            f"read{k}\t{len(r)}\t0\t{len(r)}\t+\tcontig\t{len(draft)}\t0\t{len(draft)}\t"
            f"{min(len(r), len(draft))}\t{max(len(r), len(draft))}\t255\n"
            for k, r in enumerate(reads)))
        out.update(reads=str(d / "reads.fasta"), overlaps=str(d / "overlaps.paf"),
                   draft=str(d / "draft.fasta"))
    return out


SPECIAL_READS = (0, 3, 6, 9)


def rescued_pairs():
    """(tag, band, query, target): the diagonal and the adaptive band of
    `band` cells both escape, K = 64 completes with the optimal distance."""
    out = [(f"1200 extra query bases, seed {seed}", 1024, *query_block_pair(seed))
           for seed in (9711, 9712, 9713)]
    s = pipeline_sample(None)
    out += [(f"pipeline read {k}", 256, s["read_seqs"][k], s["draft_seq"]) for k in SPECIAL_READS]
    return out


def limit_pairs():
    """(tag, query, target) that align(q, t, 64) does not complete. The first
    is also refused by the host (the band would slide several blocks per
    column). The others slide one block on almost every column, which the
    schedule covers, and escape in the traceback: a cell of the block that
    has just entered the band has no left neighbour. (A 4096-row band on the
    diagonal of a 4-9 kbp pair covers most of the rectangle, so blocks of
    missing or extra bases complete, if above the optimum; only such steep
    pairs escape at this size.)"""
    rng = random.Random(9721)
    return [(f"steep {n} x {m}, {what}", _rand_seq(rng, n), _rand_seq(rng, m))
            for n, m, what in ((64 * (64 + 8) + 100, 8, "refused"),
                               (5000, 80, "escapes in the traceback"),
                               (9000, 141, "escapes in the traceback"))]


def tiny_target_pairs():
    """(tag, query, target) with a target of one or two bases under a query
    just above the band: the band's top is at block 1 from column 1 on, so
    block 0 leaves the band before it computes anything and lane 0 has to
    start as block 64. The host admits them (one slide per column);
    align(q, t, 64) escapes in the traceback with the distance n - m."""
    rng = random.Random(9751)
    return [(f"tiny target {n} x {m}", _rand_seq(rng, n), _rand_seq(rng, m))
            for n, m in ((4097, 1), (4160, 1), (4224, 2))]


def mixed_pairs():
    """About 20 (tag, query, target) for one call: lengths from 3 to 9000
    interleaved, with a pair the K = 4 adaptive band rescues, pairs only the
    wide band rescues, the limit pairs, and one query with a single N."""
    rng = random.Random(9731)
    noise = []
    for k, t_len in enumerate((3, 9000, 65, 4097, 700, 6100, 31, 2500, 8191, 130, 5000)):
        t = _rand_seq(rng, t_len)
        q = _mutate(rng, t, 0.01, 0.005, 0.005) or "A"
        noise.append((f"noise {k} t_len={t_len}", q, t))
    tag, q, t = noise[4]
    noise[4] = (tag + ", N in the query", q[:350] + "N" + q[351:], t)
    rescued = rescued_pairs()
    special = [(r[0], r[2], r[3])
               for r in (narrow.rescued_pairs()[0], rescued[0], rescued[3], rescued[4])]
    special += limit_pairs()
    out = []
    for k, p in enumerate(noise):
        out.append(p)
        if k < len(special):
            out.append(special[k])
    assert len(special) <= len(noise)
    return out


# --------------------------------------------------------------------------
# simulator as oracle
# --------------------------------------------------------------------------

_SIM_CACHE = {}


def sim_wide(q, t):
    """What the wide band must return, in gpu_align's terms: (cigar, distance,
    status) of align(q, t, 64); a pair the host refuses is an escape without
    a distance."""
    key = (q, t)
    if key not in _SIM_CACHE:
        if not sim_myers.wave_single_slide(len(q), len(t)):
            _SIM_CACHE[key] = ("", -1, 1)
        else:
            ed, path, st = sim_myers.align(q, t, 64)
            if st == "ok":
                _SIM_CACHE[key] = (cigar_of_path(path), ed, 0)
            else:
                _SIM_CACHE[key] = ("", -1 if ed is None else ed, 1)
    return _SIM_CACHE[key]


def wide(racon, cases):
    return racon.gpu_align([(q, t) for *_, q, t in cases], band_policy="wide")


def assert_exact(cases, got):
    """Every result equals the simulator's; a completed one replays to its
    distance."""
    for (tag, *_, q, t), g in zip(cases, got):
        assert g == sim_wide(q, t), tag
        cigar, ed, status = g
        if status == 0:
            assert replay_cigar(q, t, cigar) == (len(q), len(t), ed), tag
        else:
            assert cigar == "", tag


# --------------------------------------------------------------------------
# tests
# --------------------------------------------------------------------------

def test_fits_the_band(racon):
    cases = fits_pairs()
    got = wide(racon, cases)
    assert_exact(cases, got)
    for (tag, q, t), (_, ed, status) in zip(cases, got):
        assert status == 0, tag
        assert ed == optimum(q, t), tag


def test_first_slides(racon):
    cases = slide_pairs()
    assert_exact(cases, wide(racon, cases))


def test_rescued(racon):
    cases = rescued_pairs()
    got = wide(racon, cases)
    assert_exact(cases, got)
    for band in sorted({c[1] for c in cases}):
        sub = [(c, g) for c, g in zip(cases, got) if c[1] == band]
        pairs = [(q, t) for (_, _, q, t), _ in sub]
        for policy in ("diagonal", "adaptive"):
            for ((tag, *_), _), r in zip(sub, racon.gpu_align(pairs, band_width=band,
                                                              band_policy=policy)):
                assert r[2] != 0 and r[0] == "", (tag, policy, r[1:])
        for ((tag, _, q, t), (cigar, ed, status)) in sub:
            print(f"{tag}: wide status {status} distance {ed}, optimum {optimum(q, t)}")
            assert status == 0, tag
            assert ed == optimum(q, t), tag


def test_limit(racon):
    limits = limit_pairs()
    # neighbours in the same call: a completed pair before, between and after
    fit = fits_pairs()
    tiny = tiny_target_pairs()
    limits += tiny
    cases = [fit[12], limits[0], fit[7], limits[1], slide_pairs()[1], limits[2], fit[16],
             tiny[0], fit[3], tiny[1], tiny[2], fit[9]]
    got = wide(racon, cases)
    assert_exact(cases, got)
    for (tag, q, t), (cigar, ed, status) in zip(cases, got):
        if any(tag == l[0] for l in limits):
            print(f"{tag}: status {status} distance {ed}")
            assert status != 0 and cigar == "", tag
        else:
            assert status == 0, tag
    # the refused pair has no distance either: the kernel never saw it
    assert got[1] == ("", -1, 1)
    # the tiny-target pairs ran: the forward pass's distance comes back
    for (tag, q, t), g in zip(cases, got):
        if tag.startswith("tiny target"):
            assert g == ("", len(q) - len(t), 1), tag


_MIXED_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import _racon
pairs = [tuple(p) for p in json.load(open(sys.argv[2]))]
print(json.dumps([_racon.gpu_align(pairs, band_policy="wide"),
                  _racon.gpu_align(pairs, band_width=256, band_policy="retry", wide_pass=True)]))
"""


def test_mixed_call(racon, tmp_path):
    assert "RGA_ALN_LANES" not in os.environ
    cases = mixed_pairs()
    assert 18 <= len(cases) <= 24
    pairs = [(q, t) for _, q, t in cases]
    assert sum(q.count("N") for q, _ in pairs) == 1 and not any("N" in t for _, t in pairs)
    all_wide = racon.gpu_align(pairs, band_policy="wide")
    assert_exact(cases, all_wide)

    diagonal = racon.gpu_align(pairs, band_width=256, band_policy="diagonal")
    adaptive = racon.gpu_align(pairs, band_width=256, band_policy="adaptive")
    passes = racon.gpu_align(pairs, band_width=256, band_policy="retry", wide_pass=True)
    by = {"diagonal": 0, "adaptive": 0, "wide": 0, "escaped": 0}
    for (tag, *_), d, a, w, got in zip(cases, diagonal, adaptive, all_wide, passes):
        if d[2] == 0:
            want, which = d, "diagonal"
        elif a[2] == 0:
            want, which = a, "adaptive"
        else:
            want, which = w, "wide" if w[2] == 0 else "escaped"
        assert got == want, (tag, which)
        by[which] += 1
    print(f"{len(cases)} pairs completed by: {by}")
    assert all(count > 0 for count in by.values()), by
    # without the last pass the same call is the retry policy's own
    assert racon.gpu_align(pairs, band_width=256, band_policy="retry") == \
        racon.gpu_align(pairs, band_width=256, band_policy="retry", wide_pass=False)

    args = tmp_path / "pairs.json"
    args.write_text(json.dumps(pairs))
    child = subprocess.run(
        [sys.executable, "-c", _MIXED_CHILD, os.path.dirname(racon.__file__), str(args)],
        env=dict(os.environ, RGA_ALN_LANES="64"), capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    packed = [[tuple(r) for r in results] for results in json.loads(child.stdout)]
    assert packed == [all_wide, passes]


@pytest.mark.parametrize("window_length", [64, 500])
def test_breaking_points(racon, window_length):
    """The breaking-point traceback takes the same walk: its points equal the
    CIGAR walk over the path traceback's result."""
    cases = mixed_pairs()
    pairs = [(q, t) for _, q, t in cases]
    t_begins = [(k * 137) % 1000 + 1 for k in range(len(cases))]
    q_begins = [(k * 29) % 200 + 1 for k in range(len(cases))]
    paths = racon.gpu_align(pairs, band_policy="wide")
    got = racon.gpu_breaking_points(pairs, window_length, t_begins=t_begins, q_begins=q_begins,
                                    band_policy="wide")
    assert len(got) == len(cases)
    escaped = 0
    for (tag, q, t), (cigar, ed, status), tb, qb, g in zip(cases, paths, t_begins, q_begins, got):
        want = []
        if status == 0:
            want = racon.breaking_points_from_cigar(cigar, window_length, tb, tb + len(t), qb)
        else:
            escaped += 1
        assert g == (want, ed, status), tag
    assert 0 < escaped < len(cases)
    # as a last pass the records come from whichever pass completed the pair
    paths = racon.gpu_align(pairs, band_width=256, band_policy="retry", wide_pass=True)
    got = racon.gpu_breaking_points(pairs, window_length, t_begins=t_begins, q_begins=q_begins,
                                    band_width=256, band_policy="retry", wide_pass=True)
    for (tag, q, t), (cigar, ed, status), tb, qb, g in zip(cases, paths, t_begins, q_begins, got):
        want = []
        if status == 0:
            want = racon.breaking_points_from_cigar(cigar, window_length, tb, tb + len(t), qb)
        assert g == (want, ed, status), tag


# --------------------------------------------------------------------------
# pipeline
# --------------------------------------------------------------------------

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
    assert "completed by the wide band" not in plain.stderr
    adaptive = run(base + ["--aligner-adaptive-band"] + inputs)
    assert "4 overlap(s) aligned on CPU" in adaptive.stderr, adaptive.stderr[-2000:]
    assert "completed by the wide band" not in adaptive.stderr

    first = run(base + ["--aligner-wide-band"] + inputs)
    second = run(base + ["--aligner-wide-band"] + inputs)
    both = run(base + ["--aligner-wide-band", "--aligner-adaptive-band"] + inputs)
    for p in (first, second, both):
        assert "aligned on CPU" not in p.stderr, p.stderr[-2000:]
        assert "4 overlap(s) completed by the wide band" in p.stderr, p.stderr[-2000:]
    assert first.stdout and first.stdout == second.stdout

    (tmp_path / "polished.fasta").write_text(first.stdout)
    polished = fasta_reader(tmp_path / "polished.fasta")
    assert len(polished) == 1
    polished_seq = next(iter(polished.values()))
    before = racon.edit_distance(s["draft_seq"], s["truth"])
    after = racon.edit_distance(polished_seq, s["truth"])
    print(f"edit distance to the truth: draft {before}, polished {after}")
    assert after < before

    wrapper = Path(__file__).resolve().parent.parent / "scripts" / "racon_wrapper.py"
    wrapped = run([sys.executable, str(wrapper), "--in-process", "--cudaaligner-batches", "1",
                   "--cudaaligner-band-width", "256", "-c", "1", "-t", "4",
                   "-m", "3", "-x", "-5", "-g", "-4", "--aligner-wide-band"] + inputs)
    assert "4 overlap(s) completed by the wide band" in wrapped.stderr, wrapped.stderr[-2000:]
    assert wrapped.stdout == first.stdout

    out = racon.polish(s["reads"], s["overlaps"], s["draft"], threads=4, poa_batches=1,
                       aligner_batches=1, aligner_band_width=256, aligner_wide_band=True)
    assert [seq for _, seq in out] == [polished_seq]

    with pytest.raises(ValueError):
        racon.gpu_align([("ACGT", "ACGT")], band_policy="bogus")
