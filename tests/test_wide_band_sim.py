"""CPU check of the wave kernel's schedule model and of the inputs pinned for
the wide band.

tools/sim_myers.py's align(q, t, 64) is the specification of the wide band;
align_wave() there models how src/hip/aligner_wave_kernel.hip computes it: the
step loop, lane recycling, the state handed down a lane, the step-indexed
store and the traceback over it. It must return exactly what align() returns,
and "refused" for the pairs whose band slides more than one block per column,
which the host keeps away from the kernel.

The GPU tests in test_wide_band_gpu.py hold the kernel to the simulator on
pinned pairs; this file holds those pairs to the conditions that make them
worth running. Seeds are chosen so that the conditions hold; the conditions
are not to be loosened.
"""

import random

import pytest

import test_wide_band_gpu as inputs
from test_adaptive_band_gpu import optimum, sim_result
from test_gpu_kernel_edges import replay_cigar
from test_wide_band_gpu import sim_wide

sim_myers = inputs.sim_myers


def _ids(cases):
    return [c[0] for c in cases]


def assert_wave_is_align(q, t, tag):
    want = sim_myers.align(q, t, 64)
    got = sim_myers.align_wave(q, t)
    if sim_myers.wave_single_slide(len(q), len(t)):
        assert got == want, tag
    else:
        assert got == (None, None, "refused"), tag
    return want


def test_fits_pairs():
    for tag, q, t in inputs.fits_pairs():
        assert len(q) <= 4096
        ed, path, st = assert_wave_is_align(q, t, tag)
        assert st == "ok" and ed == optimum(q, t), tag


def test_slide_pairs():
    """More than 64 query blocks: the band moves and a lane is recycled."""
    for tag, q, t in inputs.slide_pairs():
        nbt = (len(q) + 63) // 64
        assert nbt > 64, tag
        assert sim_myers.btop_of(len(t), len(q), len(t), nbt, 64) == nbt - 64, tag
        ed, path, st = assert_wave_is_align(q, t, tag)
        assert st == "ok", tag
        sim_myers.check_path(q, t, path, ed)


@pytest.mark.parametrize("case", inputs.rescued_pairs(), ids=_ids(inputs.rescued_pairs()))
def test_rescued_pairs(case):
    tag, band, q, t = case
    for adaptive in (False, True):
        narrower = sim_result(q, t, band, adaptive)
        assert narrower[2] != 0 and narrower[0] == "", (adaptive, narrower[1:])
    ed, path, st = assert_wave_is_align(q, t, tag)
    assert st == "ok" and ed == optimum(q, t)
    cigar, sim_ed, status = sim_wide(q, t)
    assert status == 0 and replay_cigar(q, t, cigar) == (len(q), len(t), ed)


def test_limit_pairs():
    cases = inputs.limit_pairs()
    results = [assert_wave_is_align(q, t, tag) for tag, q, t in cases]
    assert all(st != "ok" for _, _, st in results)
    # the first is refused by the host, the others escape in the traceback
    assert not sim_myers.wave_single_slide(len(cases[0][1]), len(cases[0][2]))
    assert len(cases[0][1]) > 64 * (64 + len(cases[0][2]))
    assert [st for _, _, st in results[1:]] == ["bandedge-tb"] * (len(cases) - 1)
    assert all(sim_myers.wave_single_slide(len(q), len(t)) for _, q, t in cases[1:])


def test_tiny_target_pairs():
    """Admitted pairs whose band top is at block 1 from the first column on:
    the model recycles lane 0 before step 1 and equals align()."""
    shapes = []
    for tag, q, t in inputs.tiny_target_pairs():
        n, m = len(q), len(t)
        shapes.append((n, m))
        assert sim_myers.wave_single_slide(n, m), tag
        assert sim_myers.btop_of(1, n, m, (n + 63) // 64, 64) == 1, tag
        assert assert_wave_is_align(q, t, tag) == (n - m, None, "bandedge-tb"), tag
        assert sim_wide(q, t) == ("", n - m, 1), tag
    assert shapes == [(4097, 1), (4160, 1), (4224, 2)]


def test_tiny_targets_on_random_pairs():
    """Targets of 1..3 bases under queries just above 4096 rows, admitted or
    refused: the corner where the band moves before some lanes have computed
    anything."""
    rng = random.Random(9743)
    admitted = 0
    for trial in range(60):
        m = rng.randint(1, 3)
        n = rng.randint(4097, 4097 + 64 * m + 63)
        q = "".join(rng.choice("ACGT") for _ in range(n))
        t = "".join(rng.choice("ACGT") for _ in range(m))
        assert_wave_is_align(q, t, f"trial {trial} n={n} m={m}")
        admitted += sim_myers.wave_single_slide(n, m)
    assert 5 <= admitted < 60


def test_mixed_set_exercises_every_pass():
    cases = inputs.mixed_pairs()
    assert 18 <= len(cases) <= 24
    lengths = [len(t) for _, _, t in cases]
    assert min(lengths) <= 8 and max(lengths) == 9000
    by = {"diagonal": 0, "adaptive": 0, "wide": 0, "escaped": 0}
    for tag, q, t in cases:
        assert_wave_is_align(q, t, tag)
        if sim_result(q, t, 256, False)[2] == 0:
            by["diagonal"] += 1
        elif sim_result(q, t, 256, True)[2] == 0:
            by["adaptive"] += 1
        else:
            by["wide" if sim_wide(q, t)[2] == 0 else "escaped"] += 1
    assert all(count > 0 for count in by.values()), by
    assert by["diagonal"] >= len(cases) // 2


def test_pipeline_sample():
    """Exactly reads 0, 3, 6 and 9 escape K = 4 under both policies against
    the draft, and K = 64 completes them optimally; the other eight complete
    under the diagonal band."""
    s = inputs.pipeline_sample(None)
    draft = s["draft_seq"]
    assert len(s["read_seqs"]) == 12
    for k, read in enumerate(s["read_seqs"]):
        diagonal = sim_myers.align(read, draft, 4)[2]
        if k in inputs.SPECIAL_READS:
            assert diagonal != "ok", k
            assert sim_myers.align(read, draft, 4, adaptive=True)[2] != "ok", k
            ed, _, st = sim_myers.align(read, draft, 64)
            assert st == "ok" and ed == optimum(read, draft), k
        else:
            assert diagonal == "ok", k


def test_wave_schedule_on_random_pairs():
    rng = random.Random(9741)
    for trial in range(40):
        m = rng.randint(1, 6000)
        t = "".join(rng.choice("ACGT") for _ in range(m))
        if trial % 4 == 0:
            q = "".join(rng.choice("ACGTN") for _ in range(rng.randint(1, 6000)))
        else:
            q = sim_myers.mutate(t, rng, (0.02, 0.06, 0.15)[trial % 3]) or "A"
        assert_wave_is_align(q, t, f"trial {trial} n={len(q)} m={m}")


def test_refusal_rule():
    """Refused pairs need a query of more than 64 blocks and more than 64
    times the target; up to there the rule admits everything."""
    rng = random.Random(9742)
    refused = 0
    for _ in range(300):
        m = rng.randint(1, 200)
        n = rng.randint(1, 100 * m)
        ok = sim_myers.wave_single_slide(n, m)
        if n <= 4096 or n <= 64 * m:
            assert ok, (n, m)
        refused += not ok
    assert refused > 0
