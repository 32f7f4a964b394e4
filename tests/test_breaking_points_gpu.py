"""The HIP aligner's breaking-point traceback mode (gpu_breaking_points).

Oracle everywhere: breaking_points_from_cigar (checked on the CPU against a
pure-Python walk in test_breaking_points.py) applied to the CIGAR gpu_align
returns for the same pair at the same band. The kernel is deterministic and
both traceback modes take the same moves, so point lists, edit distances and
statuses must be equal, not close.
"""

import json
import os
import random
import subprocess
import sys

import pytest

from test_gpu_kernel_edges import _mutate, _rand_seq, band_contract_escape_pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def require_gpu(racon):
    # torch is deliberately not imported (see test_gpu_kernel_edges.py)
    if racon.device_count() < 1:
        pytest.skip("no GPU on this host")


def _pair(rng, t_len, err=0.03):
    """(query, target): the query is the target at 3 x err edits per base."""
    t = _rand_seq(rng, t_len)
    return _mutate(rng, t, err, err, err) or rng.choice("ACGT"), t


def oracle(racon, pairs, window_length, t_begins, q_begins, band=0):
    out = []
    for (q, t), (cigar, ed, status), tb, qb in zip(
            pairs, racon.gpu_align(pairs, band_width=band), t_begins, q_begins):
        points = []
        if status == 0:
            points = racon.breaking_points_from_cigar(cigar, window_length, tb, tb + len(t), qb)
        out.append((points, ed, status))
    return out


def check(racon, cases, window_length, band=0):
    """cases: (tag, query, target, t_begin, q_begin). Returns (got, want)."""
    pairs = [(q, t) for _, q, t, _, _ in cases]
    t_begins = [c[3] for c in cases]
    q_begins = [c[4] for c in cases]
    want = oracle(racon, pairs, window_length, t_begins, q_begins, band)
    got = racon.gpu_breaking_points(pairs, window_length, t_begins=t_begins,
                                    q_begins=q_begins, band_width=band)
    assert len(got) == len(cases)
    for (tag, *_), g, w in zip(cases, got, want):
        assert g[2] == w[2], (tag, "status", g[2], w[2])
        assert g[1] == w[1], (tag, "edit distance", g[1], w[1])
        assert g[0] == w[0], (tag, "points", g[0][:6], w[0][:6])
    return got, want


def window_edge_cases(window_length):
    L = window_length
    rng = random.Random(8000 + L)
    cases = []
    for t_begin in (0, L - 1, L, L + 1):
        # first multiple of L at least 300 bases past t_begin
        mult = -(-(t_begin + 300) // L) * L
        for t_end in (mult - 1, mult, mult + 1):
            q, t = _pair(rng, t_end - t_begin)
            q_begin = rng.choice((0, 1, 250))
            cases.append((f"t_begin={t_begin} t_end={t_end} q_begin={q_begin}",
                          q, t, t_begin, q_begin))
    # a span wholly inside one window (as long as the window allows, <= 200)
    inner = min(200, max(1, L - 3))
    q, t = _pair(rng, inner)
    cases.append((f"inside one window, {inner} bases", q, t, 7 * L + (1 if L > 1 else 0), 33))
    # exactly one whole window, and a one-base span on a window's last base
    q, t = _pair(rng, L)
    cases.append(("one whole window", q, t, 2 * L, 5))
    cases.append(("one base", "A", "A", 3 * L + L - 1, 9))
    return cases


@pytest.mark.parametrize("window_length", [1, 16, 64, 500])
def test_window_edges(racon, window_length):
    """Spans that start / end on a window multiple, one below and one above,
    a span inside one window, and non-zero query origins."""
    cases = window_edge_cases(window_length)
    assert any(c[4] != 0 for c in cases)
    got, _ = check(racon, cases, window_length)
    assert all(status == 0 for _, _, status in got)
    for (tag, _, t, t_begin, _), (points, _, _) in zip(cases, got):
        n_windows = (t_begin + len(t) - 1) // window_length - t_begin // window_length + 1
        assert 2 <= len(points) <= 2 * n_windows, tag


@pytest.mark.parametrize("where", ["middle", "start", "end"])
def test_windows_without_a_match(racon, where):
    """The target carries a 60-base block the query lacks (L = 16, band 512):
    the windows under the block hold no match and are absent from the list.
    A block at the start / end exercises the leading / trailing deletion run,
    which ends the traceback in its tail rather than in its main loop.

    The block is 60 T in a target otherwise over A/C/G. A random block would
    not do: the traceback takes a diagonal move wherever that is optimal, so
    it scatters the 60 deletions between chance matches of the query's
    neighbouring bases, about one match per four block bases, and every
    window keeps a match (measured: 24 of 24 windows). T matches nothing
    around it but the few T that the 1 % mutations put into the query."""
    L = 16
    rng = random.Random(8100)
    cases = []
    for t_begin in (0, L - 1, 5 * L + 3):
        body = _rand_seq(rng, 320, "ACG")
        block = "T" * 60
        at = {"middle": 150, "start": 0, "end": 320}[where]
        t = body[:at] + block + body[at:]
        q = _mutate(rng, body, 0.01, 0.01, 0.01)
        cases.append((f"block at {where}, t_begin={t_begin}", q, t, t_begin, 4))
    got, want = check(racon, cases, L, band=512)
    for (tag, _, t, t_begin, _), (points, _, status) in zip(cases, want):
        n_windows = (t_begin + len(t) - 1) // L - t_begin // L + 1
        print(f"{tag}: {len(points) // 2} of {n_windows} windows matched")
        assert status == 0, tag
        # test-input sanity: the block empties at least two whole windows
        assert len(points) // 2 <= n_windows - 2, tag


def mixed_wave_cases():
    """78 pairs, target lengths 1..700 interleaved so that every wave mixes
    short and long lanes (lanes finish at different columns), with assorted
    origins."""
    rng = random.Random(8200)
    cases = []
    lengths = [100 + (k * 211) % 601 for k in range(64)] + list(range(1, 70, 5))
    for k, t_len in enumerate(lengths):
        q, t = _pair(rng, t_len)
        cases.append((f"pair {k} t_len={t_len}", q, t, (k * 37) % 400, (k * 13) % 90))
    return cases


_LANES_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import _racon
pairs, L, t_begins, q_begins = json.load(open(sys.argv[2]))
print(json.dumps(_racon.gpu_breaking_points([tuple(p) for p in pairs], L,
                                            t_begins=t_begins, q_begins=q_begins)))
"""


def test_mixed_wave_and_64_lane_packing(racon, tmp_path):
    """Widely differing lengths in one call, at this job size's 16
    alignments per wave here and at RGA_ALN_LANES=64 (two waves, the second
    partly filled) in a fresh process: the variable is read once per process."""
    assert "RGA_ALN_LANES" not in os.environ
    L = 64
    cases = mixed_wave_cases()
    assert len(cases) >= 70
    got, _ = check(racon, cases, L)

    args = tmp_path / "pairs.json"
    args.write_text(json.dumps([[(q, t) for _, q, t, _, _ in cases], L,
                                [c[3] for c in cases], [c[4] for c in cases]]))
    child = subprocess.run(
        [sys.executable, "-c", _LANES_CHILD, os.path.dirname(racon.__file__), str(args)],
        env=dict(os.environ, RGA_ALN_LANES="64"), capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    packed = [([tuple(p) for p in points], ed, status)
              for points, ed, status in json.loads(child.stdout)]
    assert packed == got


def test_escapes_leave_neighbours_exact(racon):
    """Band 256: pairs whose optimum lies far outside the band contract. One
    that escapes returns its non-zero status with an empty list, and the
    in-band pairs sharing its waves are untouched by it."""
    L = 64
    rng = random.Random(8300)
    cases = []
    for k, (tag, q, t) in enumerate(band_contract_escape_pairs()):
        cases.append((tag, q, t, 100 * k + 63, k))
        nq, nt = _pair(rng, 400 + 37 * k, err=0.01)
        cases.append((f"neighbour of {tag}", nq, nt, 64 * k, 3))
    got, want = check(racon, cases, L, band=256)
    escaped = [c[0] for c, w in zip(cases, want) if w[2] != 0]
    print(f"escaped at band 256: {escaped}")
    assert escaped, "test input: no pair of the escape set left the band"
    for (tag, *_), (points, ed, status) in zip(cases, got):
        if tag.startswith("neighbour"):
            assert status == 0 and points, tag
        if status != 0:
            # the distance stays what the forward pass found when the escape
            # shows only in the traceback; check() held it to gpu_align's
            assert points == [], tag


def test_record_arena_pressure(racon):
    """window_length 1 costs one record per target base. The 4 GB budget the
    entry point gives its batch sizes the record arena at about 830 k
    records (sequence arena / 64 + 2 per alignment slot); 1 300 targets of
    700 bases need 910 k, so the call is split across flushes."""
    rng = random.Random(8400)
    distinct = [_pair(rng, 700) for _ in range(26)]
    cases = []
    for k in range(1300):
        q, t = distinct[k % len(distinct)]
        cases.append((f"pair {k}", q, t, k % 5, k % 3))
    assert sum(len(c[2]) for c in cases) > 900_000
    got, _ = check(racon, cases, 1)
    assert all(status == 0 and len(points) >= 2 for points, _, status in got)


def test_positions_past_32_bits_are_refused(racon):
    """Records hold 32-bit positions with 2^32 - 1 as the no-match marker, so
    a span that reaches it can never run: status 2 (not run), as for any
    other pair the batch refuses, and its neighbour is unaffected."""
    q, t = _pair(random.Random(8500), 300)
    got = racon.gpu_breaking_points([(q, t), (q, t)], 1, t_begins=[2**32 - 200, 10])
    assert got[0] == ([], -1, 2)
    want = oracle(racon, [(q, t)], 1, [10], [0])[0]
    assert got[1] == want


_PIPELINE_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import _racon
reads, overlaps, targets, kw = json.load(open(sys.argv[2]))
print(json.dumps(_racon.polish(reads, overlaps, targets, aligner_batches=1, poa_batches=1, **kw)))
"""


@pytest.mark.parametrize("mode", ["contig", "fragment"])
def test_pipeline_routes_agree(racon, sample, tmp_path, mode):
    """polish() with the kernel's breaking points and with RGA_ALN_HOST_BP=1
    (path -> CIGAR -> host walk), each in a fresh process: byte-identical."""
    assert "RGA_ALN_HOST_BP" not in os.environ
    if mode == "contig":
        job = [sample["reads"], sample["overlaps"], sample["layout"], dict(threads=4)]
    else:
        job = [sample["reads"], sample["ava_overlaps"], sample["reads"],
               dict(threads=4, fragment_correction=True, include_unpolished=True,
                    match=1, mismatch=-1, gap=-1)]
    args = tmp_path / "job.json"
    args.write_text(json.dumps(job))
    outs = {}
    for route, env in (("device", {}), ("host", {"RGA_ALN_HOST_BP": "1"})):
        child = subprocess.run(
            [sys.executable, "-c", _PIPELINE_CHILD, os.path.dirname(racon.__file__), str(args)],
            env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        assert child.returncode == 0, child.stderr[-2000:]
        assert "align timings" in child.stderr, child.stderr[-2000:]
        outs[route] = json.loads(child.stdout)
    assert outs["device"], mode
    assert outs["device"] == outs["host"]
