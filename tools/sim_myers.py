#!/usr/bin/env python3
"""Dev-time simulator of the banded blocked-Myers kernel in
src/hip/aligner_kernel.hip — validates the recurrence, band slide, score
reconstruction and traceback logic against brute-force DP on random pairs,
for both band policies: the diagonal band (btop_of) and the adaptive band
that follows the scores (docs/DESIGN.md, "Adaptive band").
Run: python tools/sim_myers.py [K] [trials]
"""

import random
import sys

M64 = (1 << 64) - 1


def base_code(ch):
    return {"A": 0, "C": 1, "G": 2, "T": 3}.get(ch, 4)


def brute_edit(q, t):
    n, m = len(q), len(t)
    prev = list(range(m + 1))
    for i in range(1, n + 1):
        cur = [i] + [0] * m
        for j in range(1, m + 1):
            cur[j] = min(prev[j - 1] + (q[i - 1] != t[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[m]


def btop_of(j, n, m, nbt, K):
    step = (n << 32) // m  # 32.32 fixed point, as in the kernel
    center_blk = (((j * step) >> 32) & 0xFFFFFFFF) >> 6
    top = center_blk - K // 2
    hi = nbt - K if nbt > K else 0
    return max(0, min(top, hi))


def score_at(S, Pv, Mv, k):
    mask = 0 if k == 63 else (M64 << (k + 1)) & M64
    return S - (bin(Pv & mask).count("1") - bin(Mv & mask).count("1"))


def popcount(x):
    return bin(x).count("1")


def align(q, t, K, adaptive=False):
    """Returns (edit_distance, path, status). With adaptive the band top
    starts at block 0, never moves up, and before each column slides down one
    block when the band's lowest row scores below its upper boundary row (or
    when it must, to reach the last block by column m); the tops are recorded
    per column for the traceback."""
    n, m = len(q), len(t)
    nbt = (n + 63) >> 6
    hi = nbt - K if nbt > K else 0
    # peq
    nb = max(K, nbt)
    peq = [[0] * 4 for _ in range(nb)]
    for i, ch in enumerate(q):
        c = base_code(ch)
        if c < 4:
            peq[i >> 6][c] |= 1 << (i & 63)

    Pv = [M64] * K
    Mv = [0] * K
    S = [(b + 1) * 64 for b in range(K)]
    btop = 0
    tops = [0] * (m + 1)  # band top per column (adaptive: as it moved)
    tb = {}  # (j, rb) -> (Pv, Mv, S)
    for b in range(K):
        tb[(0, b)] = (Pv[b], Mv[b], S[b])

    for j in range(1, m + 1):
        c = base_code(t[j - 1])
        if adaptive:
            top = S[0] - (popcount(Pv[0]) - popcount(Mv[0]))
            bot = S[K - 1]
            slide = btop < hi and (bot < top or btop < hi - (m - j))
            btn = btop + 1 if slide else btop
        else:
            btn = btop_of(j, n, m, nbt, K)
        tops[j] = btn
        while btop < btn:
            for b in range(K - 1):
                Pv[b], Mv[b], S[b] = Pv[b + 1], Mv[b + 1], S[b + 1]
            Pv[K - 1], Mv[K - 1], S[K - 1] = M64, 0, S[K - 2] + 64
            btop += 1
        hin = 1
        for b in range(K):
            Eq = peq[btop + b][c] if (c < 4 and btop + b < nb) else 0
            hin_neg = 1 if hin < 0 else 0
            hin_pos = 1 if hin > 0 else 0
            Xv = Eq | Mv[b]
            Eq |= hin_neg
            Xh = ((((Eq & Pv[b]) + Pv[b]) & M64) ^ Pv[b]) | Eq
            Ph = Mv[b] | (~(Xh | Pv[b]) & M64)
            Mh = Pv[b] & Xh
            hout = ((Ph >> 63) & 1) - ((Mh >> 63) & 1)
            Ph = ((Ph << 1) | hin_pos) & M64
            Mh = ((Mh << 1) | hin_neg) & M64
            Pv[b] = Mh | (~(Xv | Ph) & M64)
            Mv[b] = Ph & Xv
            S[b] += hout
            hin = hout
            tb[(j, b)] = (Pv[b], Mv[b], S[b])

    rb = ((n - 1) >> 6) - btop
    if rb < 0 or rb >= K:
        return None, None, "bandedge-final"
    D = score_at(S[rb], Pv[rb], Mv[rb], (n - 1) & 63)
    ed = D

    # traceback
    path = []
    i, j = n, m
    while i > 0 and j > 0:
        babs = (i - 1) >> 6
        k = (i - 1) & 63
        if adaptive:
            btj, btj1 = tops[j], tops[j - 1]
        else:
            btj = btop_of(j, n, m, nbt, K)
            btj1 = btop_of(j - 1, n, m, nbt, K)
        rbj = babs - btj
        rbj1 = babs - btj1
        if not (0 <= rbj < K and 0 <= rbj1 < K):
            return ed, None, "bandedge-tb"
        Pvj, Mvj, _ = tb[(j, rbj)]
        Pvj1, Mvj1, S1 = tb[(j - 1, rbj1)]
        vd = 1 if (Pvj >> k) & 1 else (-1 if (Mvj >> k) & 1 else 0)
        D_left = score_at(S1, Pvj1, Mvj1, k)
        vd1 = 1 if (Pvj1 >> k) & 1 else (-1 if (Mvj1 >> k) & 1 else 0)
        D_diag = D_left - vd1
        sub = 0 if (base_code(q[i - 1]) == base_code(t[j - 1]) and base_code(q[i - 1]) < 4) else 1
        if D_diag + sub == D:
            path.append("M")
            i -= 1
            j -= 1
            D = D_diag
        elif D_left + 1 == D:
            path.append("D")
            j -= 1
            D = D_left
        elif vd == 1:
            path.append("I")
            i -= 1
            D = D - vd
        else:
            return ed, None, "stuck"
    path.extend("I" * i)
    path.extend("D" * j)
    return ed, "".join(reversed(path)), "ok"


WAVE_K = 64  # blocks of the wave kernel's band: one per lane


def wave_single_slide(n, m):
    """True when the diagonal rule at K = 64 never slides more than one block
    per column. The wave schedule needs that (a new block takes its state from
    the lane above, one step earlier); the host refuses the other pairs, which
    need n > 64 m."""
    if n <= 64 * m:
        return True  # the band centre moves at most 64 rows per column
    nbt = (n + 63) >> 6
    return all(btop_of(j, n, m, nbt, WAVE_K) - btop_of(j - 1, n, m, nbt, WAVE_K) <= 1
               for j in range(1, m + 1))


def align_wave(q, t):
    """Schedule model of src/hip/aligner_wave_kernel.hip: one wavefront per
    alignment, lane = one 64-row block of a 64-block band. Returns exactly
    align(q, t, 64) for every pair wave_single_slide() admits, and
    (None, None, "refused") for the others.

    Block B of column j is computed at step s = j + B by lane B & 63, so both
    of its inputs are one step old: (B - 1, j) on the lane above, (B, j - 1) on
    the lane itself. When the band's top passes block B its lane idles for 64
    steps and comes back as block B + 64, which starts pessimistic from the
    score the lane above hands over. Column states are stored by step,
    [s][lane], and the traceback reads that store."""
    K = WAVE_K
    n, m = len(q), len(t)
    if not wave_single_slide(n, m):
        return None, None, "refused"
    nbt = (n + 63) >> 6

    def top(j):
        return btop_of(j, n, m, nbt, K)

    def masks_of(B):  # a lane builds its block's Eq masks from q when it takes it over
        eq = [0] * 4
        for k in range(min(64, n - B * 64) if B < nbt else 0):
            c = base_code(q[B * 64 + k])
            if c < 4:
                eq[c] |= 1 << k
        return eq

    steps = m + 64 + nbt + 1  # rows of the store; the last one written is m + top(m) + 63
    store = [[None] * K for _ in range(steps)]
    blk = list(range(K))  # block each lane owns
    eqs = [masks_of(B) for B in blk]
    Pv = [M64] * K
    Mv = [0] * K
    S = [(B + 1) * 64 for B in blk]
    for lane in range(K):  # column 0: block B at step B
        store[lane][lane] = (Pv[lane], Mv[lane], S[lane])
    hout_reg = [0] * K  # what each lane sent at the end of the step before
    s_reg = [0] * K

    def recycle(lane, s):
        """After step s: the band's top passes the lane's block before the
        lane's next column, so the lane takes over the block 64 below."""
        B = blk[lane]
        jn = s + 1 - B
        if 1 <= jn <= m and B < top(jn):
            blk[lane] = B + K
            eqs[lane] = masks_of(B + K)

    last = m + top(m) + K - 1
    assert last < steps
    # step 0 computes nothing, but it has its recycle: with top(1) = 1 block 0
    # leaves the band before its first column (t_len = 1 and 4097..4160 rows,
    # 4224 x 2, ...) and lane 0 starts as block 64
    for lane in range(K):
        recycle(lane, 0)
    for s in range(1, last + 1):
        hin_in = [hout_reg[(lane - 1) % K] for lane in range(K)]  # one lane up
        s_in = [s_reg[(lane - 1) % K] for lane in range(K)]
        for lane in range(K):
            B = blk[lane]
            j = s - B
            if 1 <= j <= m:
                bt = top(j)
                assert B >= bt  # recycled in time
                if B <= bt + K - 1:
                    if B > top(j - 1) + K - 1:  # the block enters the band here
                        Pv[lane], Mv[lane] = M64, 0
                        S[lane] = (s_in[lane] - hin_in[lane]) + 64  # S_above(j - 1) + 64
                    hin = 1 if B == bt else hin_in[lane]
                    c = base_code(t[j - 1])
                    Eq = eqs[lane][c] if c < 4 else 0
                    hin_neg = 1 if hin < 0 else 0
                    hin_pos = 1 if hin > 0 else 0
                    Xv = Eq | Mv[lane]
                    Eq |= hin_neg
                    Xh = ((((Eq & Pv[lane]) + Pv[lane]) & M64) ^ Pv[lane]) | Eq
                    Ph = Mv[lane] | (~(Xh | Pv[lane]) & M64)
                    Mh = Pv[lane] & Xh
                    hout = ((Ph >> 63) & 1) - ((Mh >> 63) & 1)
                    Ph = ((Ph << 1) | hin_pos) & M64
                    Mh = ((Mh << 1) | hin_neg) & M64
                    Pv[lane] = Mh | (~(Xv | Ph) & M64)
                    Mv[lane] = Ph & Xv
                    S[lane] += hout
                    hout_reg[lane], s_reg[lane] = hout, S[lane]
                    assert store[s][lane] is None
                    store[s][lane] = (Pv[lane], Mv[lane], S[lane])
            recycle(lane, s)

    Bf = (n - 1) >> 6
    rb = Bf - top(m)
    if rb < 0 or rb >= K:
        return None, None, "bandedge-final"
    assert blk[Bf % K] == Bf
    D = score_at(S[Bf % K], Pv[Bf % K], Mv[Bf % K], (n - 1) & 63)
    ed = D

    def state(B, j):  # None when (B, j) is outside the band
        if j < 0 or j > m or not (top(j) <= B <= top(j) + K - 1):
            return None
        return store[j + B][B % K]

    path = []
    i, j = n, m
    while i > 0 and j > 0:
        B = (i - 1) >> 6
        k = (i - 1) & 63
        sj, sj1 = state(B, j), state(B, j - 1)
        if sj is None or sj1 is None:
            return ed, None, "bandedge-tb"
        Pvj, Mvj, _ = sj
        Pvj1, Mvj1, S1 = sj1
        vd = 1 if (Pvj >> k) & 1 else (-1 if (Mvj >> k) & 1 else 0)
        D_left = score_at(S1, Pvj1, Mvj1, k)
        vd1 = 1 if (Pvj1 >> k) & 1 else (-1 if (Mvj1 >> k) & 1 else 0)
        D_diag = D_left - vd1
        sub = 0 if (base_code(q[i - 1]) == base_code(t[j - 1]) and base_code(q[i - 1]) < 4) else 1
        if D_diag + sub == D:
            path.append("M")
            i -= 1
            j -= 1
            D = D_diag
        elif D_left + 1 == D:
            path.append("D")
            j -= 1
            D = D_left
        elif vd == 1:
            path.append("I")
            i -= 1
            D = D - vd
        else:
            return ed, None, "stuck"
    path.extend("I" * i)
    path.extend("D" * j)
    return ed, "".join(reversed(path)), "ok"


def check_path(q, t, path, ed):
    qi = ti = cost = 0
    for op in path:
        if op == "M":
            cost += q[qi] != t[ti]
            qi += 1
            ti += 1
        elif op == "I":
            cost += 1
            qi += 1
        else:
            cost += 1
            ti += 1
    assert qi == len(q) and ti == len(t), (qi, len(q), ti, len(t))
    assert cost == ed, (cost, ed)


def mutate(t, rng, rate):
    out = []
    for ch in t:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(rng.choice("ACGT"))
        if r < rate:
            out.append(rng.choice([c for c in "ACGT" if c != ch]))
        else:
            out.append(ch)
    return "".join(out)


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    trials = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    rng = random.Random(1)
    fails = edges = a_edges = a_exact = 0
    for trial in range(trials):
        m = rng.randint(3, 700)
        t = "".join(rng.choice("ACGT") for _ in range(m))
        if trial % 4 == 0:
            q = "".join(rng.choice("ACGTN") for _ in range(rng.randint(3, 700)))
        else:
            q = mutate(t, rng, rng.choice([0.02, 0.06, 0.15]))
        if not q:
            continue
        ref = brute_edit(q, t)
        ed, path, st = align(q, t, K)
        if st != "ok":
            edges += 1
        elif ed != ref and (ed < ref or ref <= 64 * K // 2 - 64):
            # band may truncate the optimum for wildly divergent pairs:
            # only equal-or-worse is acceptable, and only when divergent
            print(f"FAIL trial {trial}: ed={ed} ref={ref} n={len(q)} m={m}")
            fails += 1
        else:
            check_path(q, t, path, ed)
        # adaptive band: never below the optimum, a status-ok path always
        # replays to the reported distance, and a query that fits the band
        # (the band cannot move) gives exactly the diagonal result
        aed, apath, ast = align(q, t, K, adaptive=True)
        if len(q) <= 64 * K and (aed, apath, ast) != (ed, path, st):
            print(f"FAIL trial {trial}: adaptive differs at n={len(q)} <= {64 * K}")
            fails += 1
        if ast != "ok":
            a_edges += 1
        elif aed < ref:
            print(f"FAIL trial {trial}: adaptive ed={aed} below ref={ref}")
            fails += 1
        else:
            check_path(q, t, apath, aed)
            a_exact += aed == ref
        # the wave schedule is the diagonal band at K = 64, nothing else
        if align_wave(q, t) != align(q, t, WAVE_K):
            print(f"FAIL trial {trial}: align_wave differs at n={len(q)} m={m}")
            fails += 1
    # queries of more than 4096 rows, where the wave schedule recycles lanes
    for trial in range(max(1, trials // 20)):
        m = rng.randint(2000, 6000)
        t = "".join(rng.choice("ACGT") for _ in range(m))
        q = mutate(t, rng, rng.choice([0.02, 0.15]))
        q = q[:len(q) // 2] + "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 3000))) \
            + q[len(q) // 2:]
        if align_wave(q, t) != align(q, t, WAVE_K):
            print(f"FAIL long trial {trial}: align_wave differs at n={len(q)} m={m}")
            fails += 1
    # tiny targets under queries just above the band: the band's top moves at
    # column 1 or 2, before some lanes have computed anything
    for trial in range(max(3, trials // 5)):
        m = rng.randint(1, 3)
        n = rng.randint(4097, 4097 + 64 * m + 63)
        q = "".join(rng.choice("ACGT") for _ in range(n))
        t = "".join(rng.choice("ACGT") for _ in range(m))
        want = align(q, t, WAVE_K) if wave_single_slide(n, m) else (None, None, "refused")
        if align_wave(q, t) != want:
            print(f"FAIL tiny-target trial {trial}: align_wave differs at n={n} m={m}")
            fails += 1
    print(f"K={K}: {trials} trials, {fails} fails, {edges} band-edge (diagonal), "
          f"{a_edges} band-edge / {a_exact} optimal (adaptive)")
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main())
