"""breaking_points_from_cigar against a short pure-Python walk (CPU only).

The C++ walk (rga::breaking_points_from_cigar, the body of what used to be
Overlap::find_breaking_points_from_cigar) closes windows at precomputed
window-end positions. The reference here groups matches by `t // L` instead,
so the two share no logic: per window_length slice of the target, aligned to
coordinate 0, the first matched (t, q) and the last matched (t + 1, q + 1).

The same helpers build the expectations of test_breaking_points_gpu.py.
"""

import random
import re

import pytest

_RUN = re.compile(r"(\d+)([MID])")


def py_breaking_points(cigar, window_length, t_begin, t_end, q_begin):
    assert "".join(n + op for n, op in _RUN.findall(cigar)) == cigar
    windows = {}
    t, q = t_begin, q_begin
    for num, op in _RUN.findall(cigar):
        for _ in range(int(num)):
            if op == "M":
                first_last = windows.setdefault(t // window_length, [(t, q), None])
                first_last[1] = (t + 1, q + 1)
                t += 1
                q += 1
            elif op == "I":
                q += 1
            else:
                t += 1
    assert t == t_end, (t, t_end)
    out = []
    for k in sorted(windows):
        out.extend(windows[k])
    return out


def random_cigar(rng, t_len, lead=None, trail=None, weights=(6, 1, 1), max_run=None):
    """Random M/I/D runs consuming exactly t_len target bases; lead / trail
    are (op, length) runs forced at the ends (their D bases count)."""
    fixed = sum(r[1] for r in (lead, trail) if r and r[0] == "D")
    assert fixed <= t_len
    runs = [lead] if lead else []
    left = t_len - fixed
    while left > 0:
        op = rng.choices("MID", weights)[0]
        if runs and runs[-1][0] == op:
            continue
        n = rng.randint(1, max_run or max(1, t_len // 6))
        if op != "I":
            n = min(n, left)
            left -= n
        runs.append((op, n))
    if trail:
        if runs and runs[-1][0] == trail[0]:
            runs[-1] = (trail[0], runs[-1][1] + trail[1])
        else:
            runs.append(trail)
    return "".join(f"{n}{op}" for op, n in runs)


def cigar_t_len(cigar):
    return sum(int(n) for n, op in _RUN.findall(cigar) if op != "I")


def span_cases(window_length):
    """(t_begin, t_len): t_begin on a window multiple, one below, one above
    and 0; t_end on a multiple, one below and one above; and a span inside
    one window (when a window can hold one)."""
    L = window_length
    cases = []
    for t_begin in (0, L - 1, L, L + 1, 3 * L + L // 2):
        base = (t_begin // L + 4) * L
        for t_end in (base - 1, base, base + 1):
            cases.append((t_begin, t_end - t_begin))
    if L >= 4:
        cases.append((2 * L + 1, L - 2))
        cases.append((2 * L, L))
    cases.append((5 * L, 1))
    return cases


@pytest.mark.parametrize("window_length", [1, 2, 7, 16, 64, 500])
def test_random_cigars(racon, window_length):
    rng = random.Random(100 + window_length)
    L = window_length
    n_checked = 0
    for t_begin, t_len in span_cases(L):
        for q_begin in (0, 37):
            cigar = random_cigar(rng, t_len, max_run=max(2, L // 2 + 3))
            want = py_breaking_points(cigar, L, t_begin, t_begin + t_len, q_begin)
            got = racon.breaking_points_from_cigar(cigar, L, t_begin, t_begin + t_len, q_begin)
            assert got == want, (cigar, L, t_begin, t_len, q_begin)
            n_checked += 1
    assert n_checked >= 30


@pytest.mark.parametrize("window_length", [1, 16, 64])
@pytest.mark.parametrize("t_begin_off", [-1, 0, 1])
def test_deletion_run_of_three_windows(racon, window_length, t_begin_off):
    """A deletion run spanning three whole windows: those windows are absent
    from the list, wherever the run sits relative to the slices."""
    rng = random.Random(200 + window_length)
    L = window_length
    t_begin = 2 * L + t_begin_off
    for shift in (0, 1, L // 2):
        head = 2 * L + shift
        cigar = f"{head}M{3 * L + (2 if L > 1 else 0)}D3I{2 * L + 1}M"
        t_end = t_begin + cigar_t_len(cigar)
        want = py_breaking_points(cigar, L, t_begin, t_end, 5)
        got = racon.breaking_points_from_cigar(cigar, L, t_begin, t_end, 5)
        assert got == want, (cigar, t_begin)
        n_windows = (t_end - 1) // L - t_begin // L + 1
        assert len(got) // 2 <= n_windows - 2, "no window was skipped"
    cigar = random_cigar(rng, 9 * L, weights=(3, 1, 3), max_run=3 * L + 1)
    t_end = t_begin + 9 * L
    assert racon.breaking_points_from_cigar(cigar, L, t_begin, t_end, 0) == \
        py_breaking_points(cigar, L, t_begin, t_end, 0)


@pytest.mark.parametrize("window_length", [1, 16, 500])
@pytest.mark.parametrize("lead", [("I", 5), ("D", 5), ("D", 40), None])
@pytest.mark.parametrize("trail", [("I", 3), ("D", 3), ("D", 40), None])
def test_leading_and_trailing_runs(racon, window_length, lead, trail):
    rng = random.Random(300 + window_length)
    L = window_length
    for t_begin, t_len in ((0, 120), (L - 1, 3 * L + 100), (L + 1, 97)):
        cigar = random_cigar(rng, t_len, lead=lead, trail=trail, max_run=9)
        t_end = t_begin + cigar_t_len(cigar)
        want = py_breaking_points(cigar, L, t_begin, t_end, 11)
        got = racon.breaking_points_from_cigar(cigar, L, t_begin, t_end, 11)
        assert got == want, (cigar, t_begin)


def test_no_match_at_all(racon):
    assert racon.breaking_points_from_cigar("4I9D", 4, 3, 12, 0) == []
    assert racon.breaking_points_from_cigar("9D4I", 4, 3, 12, 0) == []


def test_rejects_inconsistent_span(racon):
    with pytest.raises(ValueError):
        racon.breaking_points_from_cigar("10M", 0, 0, 10, 0)
    with pytest.raises(ValueError):
        racon.breaking_points_from_cigar("10M", 4, 0, 11, 0)
    with pytest.raises(ValueError):
        racon.breaking_points_from_cigar("10M", 4, 5, 5, 0)
