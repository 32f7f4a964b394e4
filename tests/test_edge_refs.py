"""CPU checks of the reference helpers used by test_gpu_kernel_edges.py.

The GPU tests compare the HIP aligner with np_edit_distance (a plain NumPy
row DP) where the pair is short enough and with racon.edit_distance
otherwise; this file ties the two together on random pairs and on the exact
aligner inputs of the GPU tests, and checks the CIGAR replay helper.
"""

import random

import pytest

import test_gpu_kernel_edges as edges


def test_np_edit_distance_matches_native_on_random_pairs(racon):
    rng = random.Random(17)
    assert edges.np_edit_distance("", "") == 0
    assert edges.np_edit_distance("", "ACG") == 3
    assert edges.np_edit_distance("ACGTNNNNACGT", "ACGTNNNNACGT") == 0
    assert edges.np_edit_distance("ACGT", "AGT") == 1
    for k in range(50):
        alphabet = "ACGTN" if k % 3 == 0 else "ACGT"
        a = edges._rand_seq(rng, rng.randint(1, 400), alphabet)
        if k % 2:
            b = edges._mutate(rng, a, 0.05, 0.05, 0.05) or "A"
        else:
            b = edges._rand_seq(rng, rng.randint(1, 400), alphabet)
        if k % 6 == 0:
            at = rng.randrange(len(a))
            a = a[:at] + "NNNN" + a[at:]
        assert edges.np_edit_distance(a, b) == racon.edit_distance(a, b), (k, a, b)


@pytest.mark.parametrize("band", edges.BANDS)
def test_np_edit_distance_on_boundary_inputs(racon, band):
    K = band // 64
    bound = edges.band_exact_bound(K)
    pairs = edges.aligner_boundary_pairs(band) + edges.band_contract_exact_pairs(band)
    if band == 256:
        pairs += edges.band_contract_escape_pairs()
    for tag, q, t in pairs:
        opt = edges.np_edit_distance(q, t)
        assert opt == racon.edit_distance(q, t), (band, tag)
        if tag.startswith("mismatch"):
            assert opt == max(len(q), len(t)), tag
        if tag.startswith("homopolymer"):
            assert opt == 5, tag
        if tag.startswith(("mut", "identical", "del")):
            # these sit inside the band contract: optimum under the bound
            assert opt <= bound, (band, tag, opt, bound)
        if tag.startswith("escape"):
            assert opt > bound, (tag, opt)


def test_np_edit_distance_on_mixed_wave_inputs(racon):
    for tag, q, t in edges.mixed_wave_pairs():
        opt = edges.np_edit_distance(q, t)
        assert opt == racon.edit_distance(q, t), tag
        if tag.startswith("long"):
            assert opt <= edges.band_exact_bound(8), (tag, opt)


def test_np_edit_distance_on_lane_packing_inputs(racon):
    pairs = edges.lane_packing_pairs()
    assert len(pairs) == 16400
    for k, (q, t) in enumerate(pairs):
        assert 1 <= len(t) <= 130 and len(q) >= 1
        assert edges.np_edit_distance(q, t) == racon.edit_distance(q, t), k


def test_replay_cigar(racon):
    assert edges.replay_cigar("ACGT", "ACGT", "4M") == (4, 4, 0)
    assert edges.replay_cigar("ACGT", "AGGT", "4M") == (4, 4, 1)
    assert edges.replay_cigar("ACNT", "ACNT", "4M") == (4, 4, 0)  # N matches N
    assert edges.replay_cigar("ACGT", "AT", "1M2I1M") == (4, 2, 2)
    assert edges.replay_cigar("AT", "ACGT", "1M2D1M") == (2, 4, 2)
    assert edges.replay_cigar("ACGT", "ACGT", "2M") == (2, 2, 0)  # caller checks lengths
    for bad in ("4X", "4=", "3M1S", "M", "4M3", "2M 2M"):
        with pytest.raises(ValueError):
            edges.replay_cigar("ACGT", "ACGT", bad)
    with pytest.raises(ValueError):
        edges.replay_cigar("ACGT", "ACGT", "5M")
    # the native CIGAR of a random pair replays to the native distance
    rng = random.Random(3)
    t = edges._rand_seq(rng, 500)
    q = edges._mutate(rng, t, 0.03, 0.03, 0.03)
    cigar = racon.align_cigar(q, t)
    assert edges.replay_cigar(q, t, cigar) == (len(q), len(t), racon.edit_distance(q, t))


def test_poa_window_node_counts(racon):
    """The CPU-only node-count binding: a backbone with identical layers
    keeps exactly one node per base; an insertion adds its bases."""
    bb = "ACGTTGCAAGGCTTAACCGGTTAACGGATCCA" * 4
    same = [(bb, "!" * len(bb), 0, 0)] + [(bb, "", 0, len(bb) - 1)] * 3
    ins = bb[:60] + "TTTTT" + bb[60:]
    grown = same + [(ins, "", 0, len(bb) - 1)]
    under = same[:2]
    counts = racon.poa_window_node_counts([same, grown, under])
    assert counts[0] == len(bb)
    assert len(bb) < counts[1] <= len(bb) + 5
    assert counts[2] == 0  # fewer than three layers: no graph is built
