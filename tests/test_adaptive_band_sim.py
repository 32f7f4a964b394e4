"""CPU check of the adaptive-band policy and of the inputs pinned for it.

tools/sim_myers.py is the specification of both band policies. The GPU tests
in test_adaptive_band_gpu.py hold the kernel to the simulator on pinned pairs;
this file holds those pairs to the conditions that make them exercise the
feature: a "rescued" pair escapes the diagonal band and is completed with the
optimal distance by the adaptive one, a "limit" pair is beyond the adaptive
band, a "same" pair gives identical results under both. Seeds are chosen so
that the conditions hold; the conditions are not to be loosened.
"""

import random

import pytest

import test_adaptive_band_gpu as inputs
from test_adaptive_band_gpu import optimum, sim_result
from test_gpu_kernel_edges import replay_cigar

sim_myers = inputs.sim_myers


def _ids(cases):
    return [c[0] for c in cases]


@pytest.mark.parametrize("case", inputs.rescued_pairs(), ids=_ids(inputs.rescued_pairs()))
def test_rescued_pairs(case):
    tag, band, q, t = case
    diagonal = sim_result(q, t, band, False)
    assert diagonal[2] != 0 and diagonal[0] == "", diagonal[1:]
    cigar, ed, status = sim_result(q, t, band, True)
    assert status == 0
    assert ed == optimum(q, t)
    assert replay_cigar(q, t, cigar) == (len(q), len(t), ed)


@pytest.mark.parametrize("case", inputs.limit_pairs(), ids=_ids(inputs.limit_pairs()))
def test_limit_pairs(case):
    tag, band, q, t = case
    cigar, ed, status = sim_result(q, t, band, True)
    assert status != 0 or ed > optimum(q, t)
    if status == 0:  # never below the optimum, and the path costs what it says
        assert replay_cigar(q, t, cigar) == (len(q), len(t), ed)


def test_same_pairs():
    for tag, band, q, t in inputs.same_pairs():
        assert len(q) <= band
        got = sim_myers.align(q, t, band // 64, adaptive=True)
        assert got == sim_myers.align(q, t, band // 64), tag
        assert got[2] == "ok" and got[0] == optimum(q, t), tag


def test_slide_pairs():
    """The shortest queries that can move the band: sound under the adaptive
    policy, and the forced slides of m = n/2 are really taken."""
    forced = 0
    for tag, band, q, t in inputs.slide_pairs():
        K = band // 64
        assert (len(q) + 63) // 64 > K, tag
        cigar, ed, status = sim_result(q, t, band, True)
        if status == 0:
            assert replay_cigar(q, t, cigar) == (len(q), len(t), ed), tag
            assert ed >= optimum(q, t), tag
        forced += len(t) < len(q)
    assert forced >= 3


def test_mixed_set_exercises_both_passes():
    cases = inputs.mixed_pairs()
    assert 75 <= len(cases) <= 90
    assert {band for _, band, _, _ in cases} == {256}
    escaped = [c for c in cases if sim_result(c[2], c[3], 256, False)[2] != 0]
    completed = [c for c in escaped if sim_result(c[2], c[3], 256, True)[2] == 0]
    assert 0 < len(completed) < len(escaped)
    # the noise pairs stay in the diagonal band: the second pass is a minority
    assert len(escaped) <= 10


def test_n_in_query_pair():
    tag, band, q, t = inputs.n_in_query_pair()
    assert q.count("N") == 1 and "N" not in t
    assert sim_result(q, t, band, False)[2] != 0
    cigar, ed, status = sim_result(q, t, band, True)
    assert status == 0 and ed == optimum(q, t)


def test_pipeline_sample(tmp_path):
    """The four reads with extra blocks escape the 256 diagonal band against
    the draft and complete under the adaptive one; the other eight complete
    under the diagonal band."""
    s = inputs.pipeline_sample(tmp_path)
    draft = s["draft_seq"]
    assert len(s["read_seqs"]) == 12
    for k, read in enumerate(s["read_seqs"]):
        diagonal = sim_myers.align(read, draft, 4)[2]
        if k % 3 == 0:
            assert diagonal != "ok", k
            assert sim_myers.align(read, draft, 4, adaptive=True)[2] == "ok", k
        else:
            assert diagonal == "ok", k


def test_policy_properties_on_random_pairs():
    """Never below the optimum; a status-ok path replays to its distance; a
    query that fits the band gives the diagonal result."""
    rng = random.Random(9601)
    for trial in range(40):
        K = rng.choice((4, 8))
        m = rng.randint(1, 900)
        t = "".join(rng.choice("ACGT") for _ in range(m))
        if trial % 4 == 0:
            q = "".join(rng.choice("ACGTN") for _ in range(rng.randint(1, 900)))
        else:
            q = sim_myers.mutate(t, rng, rng.choice([0.02, 0.06, 0.15])) or "A"
        ed, path, st = sim_myers.align(q, t, K, adaptive=True)
        if len(q) <= 64 * K:
            assert (ed, path, st) == sim_myers.align(q, t, K)
        if st == "ok":
            sim_myers.check_path(q, t, path, ed)
            # the simulator's N matches nothing; byte equality can only be cheaper
            assert ed >= optimum(q, t)
