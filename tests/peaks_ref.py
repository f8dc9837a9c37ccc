"""numpy restatement of the score-row peaks (include/rslf_hip.h, rslf_peaks), written from the rule's text, not from the
kernel: candidates by the definition over the whole row, winner and runner-up by a scan of the candidate list, every float
operation wrapped in np.float32.  Also the hand-worked rows the CPU, C++ and GPU tests share, and the planted-line field."""
import numpy as np

F = np.float32


def peaks_ref(s, lo, hi):
    """(idx, score, disp, runner_idx, runner_score) of one row s[0..D-1] with range [lo, hi]."""
    s = np.asarray(s, dtype=np.float32)
    D = len(s)
    lo, hi = F(lo), F(hi)
    cand = [j for j in range(D) if (j == 0 or s[j] > s[j - 1]) and (j == D - 1 or s[j] >= s[j + 1])]
    i1 = cand[0]
    for j in cand:
        if s[j] > s[i1]:
            i1 = j
    others = [j for j in cand if j != i1]
    i2 = -1
    for j in others:
        if i2 < 0 or s[j] > s[i2]:
            i2 = j
    s1 = s[i1]
    s2 = s[i2] if i2 >= 0 else F(0)
    rng = F(hi - lo)
    denom = F(D - 1)
    Dd = F(lo + F(F(F(i1) * rng) / denom))
    if i1 == 0 or i1 == D - 1:
        delta = F(0)
    else:
        a, c = s[i1 - 1], s[i1 + 1]
        num = F(a - c)
        t = F(a + c)
        bb = F(s1 + s1)
        den = F(t - bb)
        den2 = F(den + den)
        delta = F(0) if den2 == 0 else F(num / den2)
        delta = min(max(delta, F(-0.5)), F(0.5))
    step = F(rng / denom)
    disp = F(Dd + F(delta * step))
    return int(i1), F(s1), F(disp), int(i2), F(s2)


def branches(s):
    """Which branches of the rule a row takes: a set of names (the GPU test asserts its inputs hit every one)."""
    s = np.asarray(s, dtype=np.float32)
    D = len(s)
    i1, s1, _, i2, s2 = peaks_ref(s, 0.0, 1.0)
    out = {"first" if i1 == 0 else "last" if i1 == D - 1 else "interior"}
    if 0 < i1 < D - 1:
        a, c = s[i1 - 1], s[i1 + 1]
        den = F(F(a + c) - F(s1 + s1))
        den2 = F(den + den)
        if den2 == 0:
            out.add("den2_zero")
        elif abs(np.float64(F(F(a - c) / den2))) >= 0.5:
            out.add("clamp")
        else:
            out.add("fitted")
    out.add("no_runner" if i2 < 0 else "tied_runner" if s2 == s1 else "runner")
    out.add("winner_%d" % i1)
    return out


# Rows worked by hand: (name, row, lo, hi, idx, score, disp, runner_idx, runner_score).  Scores are small dyadic numbers so
# that every step is exact in binary32 and can be checked on paper.
_E = float(np.float32(1) - np.float32(2.0 ** -24))   # the float below 1: fl(_E + 1) = 2 (a tie, to even) = 1 + 1
HAND = [
    # winner at 0: a falling row, no other candidate; delta = 0, Dd = lo
    ("winner_first", [4, 3, 2, 1], -1.0, 2.0, 0, 4.0, -1.0, -1, 0.0),
    # winner at D-1: a rising row; Dd = -1 + (3 * 3) / 3 = 2
    ("winner_last", [1, 2, 3, 4], -1.0, 2.0, 3, 4.0, 2.0, -1, 0.0),
    # interior, the only candidate is 2: a = 1, s1 = 4, c = 3: num = -2, t = 4, bb = 8, den = -4, den2 = -8, delta = 0.25;
    # Dd = 0 + (2 * 4) / 4 = 2, step = 1, disp = 2.25
    ("interior", [0, 1, 4, 3, 2], 0.0, 4.0, 2, 4.0, 2.25, -1, 0.0),
    # interior with a runner-up: candidates 1 (5) and 4 (3); a = 2, c = 4: num = -2, t = 6, bb = 10, den = -4, den2 = -8,
    # delta = 0.25; Dd = 0 + (1 * 5) / 5 = 1, step = 1
    ("runner", [2, 5, 4, 0, 3, 1], 0.0, 5.0, 1, 5.0, 1.25, 4, 3.0),
    # a negative offset: the only candidate is 2; a = 3, c = 1: num = 2, t = 4, bb = 8, den = -4, den2 = -8, delta = -0.25;
    # Dd = 2, step = 1.  (delta = -0.5 exactly would need a == s1, and then i1 - 1 is the candidate, not i1.)
    ("delta_negative", [0, 3, 4, 1], 0.0, 3.0, 2, 4.0, 1.75, -1, 0.0),
    # an all-equal row: one plateau, candidate 0 alone
    ("all_equal", [2, 2, 2, 2], -1.0, 1.0, 0, 2.0, -1.0, -1, 0.0),
    # den2 == 0 in the interior: candidate 1 (1 > E, 1 >= 1): a = E, c = 1: t = fl(E + 1) = 2, bb = 2, den = 0 -> delta = 0
    ("den2_zero", [_E, 1, 1, 0], 0.0, 3.0, 1, 1.0, 1.0, -1, 0.0),
    # delta exactly +0.5, c == s1 (a plateau of two): a = 0: num = -2, t = 2, bb = 4, den = -2, den2 = -4; Dd = 1, step = 1
    ("delta_plus_half", [0, 2, 2, 0], 0.0, 3.0, 1, 2.0, 1.5, -1, 0.0),
    # D = 2: either winner is at an end of the grid
    ("two_equal", [1, 1], 0.5, 0.75, 0, 1.0, 0.5, -1, 0.0),
    ("two_rising", [1, 2], 0.5, 0.75, 1, 2.0, 0.75, -1, 0.0),
    # a runner-up tied with the winner: candidates 1 and 3, both 5: the first wins, the later one is the runner-up;
    # a = c = 1: num = 0 -> delta = 0
    ("tied_runner", [1, 5, 1, 5, 0], 0.0, 4.0, 1, 5.0, 1.0, 3, 5.0),
    # plateaus: candidates 1 (first of the 3s) and 5 (first of the 2s); a = 1, c = 3: num = -2, t = 4, bb = 6, den = -2,
    # den2 = -4, delta = 0.5; Dd = 0 + (1 * 7) / 7 = 1, step = 1
    ("plateaus", [1, 3, 3, 3, 1, 2, 2, 0], 0.0, 7.0, 1, 3.0, 1.5, 5, 2.0),
    # three other candidates (2, 4, 6) of which the middle one is the largest; lo == hi: disp is lo
    ("flat_range", [9, 0, 2, 0, 6, 0, 4], 0.3, 0.3, 0, 9.0, float(F(0.3)), 4, 6.0),
    # the winner comes last, the earlier best becomes the runner-up: candidates 1 (3) and 5 (7; 3 is none: 2 < 4);
    # a = 4, c = 6: num = -2, t = 10, bb = 14, den = -4, den2 = -8, delta = 0.25; Dd = 5, step = 1
    ("late_winner", [0, 3, 0, 2, 4, 7, 6], 0.0, 6.0, 5, 7.0, 5.25, 1, 3.0),
]


def hand_rows():
    return [(n, np.asarray(r, np.float32), F(lo), F(hi), i1, F(s1), F(d), i2, F(s2)) for n, r, lo, hi, i1, s1, d, i2, s2 in HAND]


def planted_epi(d_true, S=9, U=96, s_hat=4):
    """The planted-line field: a smooth texture seen under disparity d_true, [S, U] float32."""
    rng = np.random.default_rng(11)
    fr = rng.uniform(0.05, 0.6, 6)
    ph = rng.uniform(0, 6.28, 6)
    am = rng.uniform(0.3, 1, 6)

    def tex(x):
        return 0.5 + 0.4 * (am * np.sin(fr * x[..., None] + ph)).sum(axis=-1) / am.sum()

    s = np.arange(S, dtype=np.float64)[:, None]
    u = np.arange(U, dtype=np.float64)[None, :]
    return tex(u - (s_hat - s) * d_true).astype(np.float32)
