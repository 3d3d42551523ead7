"""Test infrastructure for forced alignment on the token-and-duration (TDT) lattice: the float64 NumPy restatement of the definition
in include/rnnt_tdt_align.h, written from its equations on top of tests/tdt_cases.py weights() -- a dense max-plus recurrence over
the nodes with the tie rule and the margins of its decisions, a back-trace, a scorer for any list of (frame, duration) per label, a
brute-force maximum for tiny lattices -- and the input builders the CPU and GPU tests share.  Nothing here touches the engine.

Nodes (t, u), 0 <= t < T, 0 <= u <= L, and the terminal (T, L).  Into node (t, u), for each i with d = durations[i], in increasing i:
    the blank arrival from (t-d, u),    v(t-d, u)   + wb[t-d, u, i],    iff d > 0 and t-d >= 0 (the node itself exists)
    the label arrival from (t-d, u-1),  v(t-d, u-1) + wl[t-d, u-1, i],  iff u >= 1, t < T and t-d >= 0
A candidate replaces the incumbent only if it is STRICTLY greater.  The decision code of a node is 2 i + (1 for the label arrival)."""
from __future__ import annotations

import numpy as np

from tests import tdt_cases as tc

NEG = -np.inf


# ---- the restatement --------------------------------------------------------------------------------------------------
def viterbi(wb, wl, durations):
    """(v [T+1, L+1], code [T+1, L+1] int (-1: no arrival), margin [T+1, L+1]): margin = best minus second-best candidate of the
    node, +inf with fewer than two candidates above -inf.  Row T holds the terminal's column L alone."""
    T, U, _ = wb.shape
    L = U - 1
    v = np.full((T + 1, U), NEG)
    code = np.full((T + 1, U), -1, dtype=np.int64)
    margin = np.full((T + 1, U), np.inf)
    v[0, 0] = 0.0
    for t in range(T + 1):
        for u in (range(U) if t < T else (L,)):  # d = 0 label edges go to (t, u + 1): row-major order meets sources first
            if t == 0 and u == 0:
                continue
            best, second, c = NEG, NEG, -1
            for i, d in enumerate(durations):
                ts = t - d
                if ts < 0:
                    break
                cands = []
                if d > 0:
                    cands.append((2 * i, v[ts, u] + wb[ts, u, i]))
                if u >= 1 and t < T:
                    cands.append((2 * i + 1, v[ts, u - 1] + wl[ts, u - 1, i]))
                for k, cand in cands:
                    if cand > best:
                        best, second, c = cand, best, k
                    elif cand > second:
                        second = cand
            v[t, u], code[t, u] = best, c
            if second > NEG:
                margin[t, u] = best - second
    return v, code, margin


def backtrace(code, durations):
    """From (T, L): (frames [L], durs [L], idx [L] duration indices, the nodes on the path as (t, u), last node first)."""
    T, L = code.shape[0] - 1, code.shape[1] - 1
    t, u = T, L
    frames, durs, idx = np.full(L, -1, np.int64), np.full(L, -1, np.int64), np.full(L, -1, np.int64)
    nodes = [(t, u)]
    while (t, u) != (0, 0):
        c = int(code[t, u])
        assert c >= 0, (t, u)
        i, d = c >> 1, durations[c >> 1]
        if c & 1:
            u -= 1
            frames[u], durs[u], idx[u] = t - d, d, i
        t -= d
        nodes.append((t, u))
    return frames, durs, idx, nodes


def _best_blank_fill(wb, durations, u, ta, tb, T, L):
    """The best chain of blank edges in column u from frame ta to frame tb (0 for ta == tb, -inf when there is none)."""
    g = np.full(tb - ta + 1, NEG)
    g[0] = 0.0
    for t in range(ta + 1, tb + 1):
        if not (t < T or (t == T and u == L)):
            continue
        for i, d in enumerate(durations):
            if d > 0 and t - d >= ta:
                g[t - ta] = max(g[t - ta], g[t - d - ta] + wb[t - d, u, i])
    return g[-1]


def score_path(wb, wl, durations, frames, durs):
    """Float64 value of the best path that emits label u in frame frames[u] over duration durs[u]: the label edges are given, every
    gap between them (and the way to the terminal) is filled with its best chain of blank edges -- what an optimal aligner does."""
    T, U, _ = wb.shape
    L = U - 1
    frames, durs = [int(f) for f in frames], [int(d) for d in durs]
    assert len(frames) == L == len(durs)
    total, t = 0.0, 0
    for u in range(L):
        f, d = frames[u], durs[u]
        assert d in durations and t <= f and f + d < T, (u, f, d, t, T)
        total += _best_blank_fill(wb, durations, u, t, f, T, L) + wl[f, u, list(durations).index(d)]
        t = f + d
    return total + _best_blank_fill(wb, durations, L, t, T, T, L)


def brute_force_best(wb, wl, durations):
    """max over every path from (0, 0) to the terminal, enumerated edge by edge; -inf when there is none."""
    T, U, _ = wb.shape
    L = U - 1
    best = [NEG]

    def walk(t, u, s):
        if (t, u) == (T, L):
            best[0] = max(best[0], s)
            return
        for i, label, (t2, u2) in tc.out_edges(t, u, T, L, durations):
            walk(t2, u2, s + (wl if label else wb)[t, u, i])

    walk(0, 0, 0.0)
    return best[0]


def restate(acts_b, labels_b, T_b, L_b, durations, blank=0, sigma=0.0):
    """One utterance: dict(frames, durs, score, logp, min_margin, wb, wl) of the restatement's best path.  No path: score -inf,
    frames and durs -1, logp 0."""
    x = np.asarray(acts_b, np.float64)[:T_b, : L_b + 1]
    lp, ld, wb, wl, y = tc.weights(x, np.asarray(labels_b)[:L_b], durations, blank, sigma)
    v, code, margin = viterbi(wb, wl, durations)
    if v[T_b, L_b] == NEG:
        return dict(frames=np.full(L_b, -1, np.int64), durs=np.full(L_b, -1, np.int64), score=NEG, logp=np.zeros(L_b),
                    min_margin=np.inf, wb=wb, wl=wl)
    frames, durs, idx, nodes = backtrace(code, durations)
    mm = min([margin[t, u] for t, u in nodes] + [np.inf])
    logp = np.array([lp[f, u, y[u]] + ld[f, u, i] for u, (f, i) in enumerate(zip(frames, idx))])
    return dict(frames=frames, durs=durs, score=float(v[T_b, L_b]), logp=logp, min_margin=float(mm), wb=wb, wl=wl)


def check_valid_path(frames_row, durs_row, T_b, L_b, durations):
    """One utterance's token_frames / token_durations rows (padded with -1): frames within [0, T), durations from the set, each label
    no earlier than where the one before it landed (equal frames only across d = 0), a label edge never landing on T, -1 past L."""
    fr, du = np.asarray(frames_row), np.asarray(durs_row)
    assert (fr[L_b:] == -1).all() and (du[L_b:] == -1).all(), (fr, du, L_b)
    t = 0
    for u in range(L_b):
        assert int(du[u]) in durations and t <= fr[u] and fr[u] + du[u] < T_b, (u, fr, du, T_b)
        t = int(fr[u] + du[u])


# ---- inputs -----------------------------------------------------------------------------------------------------------
def planted_case(seed, B, T, L, V, durations, gain=20.0, blank=0):
    """N(0,1) logits plus `gain` on the chosen token and the chosen duration of each cell of one planted path per utterance (full
    lengths).  The path is a random walk: label u is due at a random frame, a due label is emitted over a random duration that leaves
    room for the rest, blanks jump a random duration otherwise, and the last edge is a blank landing on T.
    Returns (acts, labels, il, ll, frames [B, L], durs [B, L])."""
    D = len(durations)
    acts, labels, il, ll = tc.full_case(B, T, L, V, D, seed, blank=blank)
    rng = np.random.default_rng(seed + 1)
    dmin = durations[0]
    frames, durs = np.full((B, max(L, 1)), -1, np.int64), np.full((B, max(L, 1)), -1, np.int64)
    assert L * dmin <= T - 1
    for b in range(B):
        due = np.sort(rng.integers(0, T, size=L)) if L else np.zeros(0, int)
        t = u = 0
        while True:
            room = lambda t2, left: t2 + left * dmin <= T - 1  # noqa: E731 -- `left` labels still fit after landing on t2
            blanks = [i for i, d in enumerate(durations) if d > 0 and (room(t + d, L - u) if u < L else t + d <= T)]
            if u < L and (due[u] <= t or not blanks):
                fits = [i for i, d in enumerate(durations) if room(t + d, L - u - 1)]
                i = fits[int(rng.integers(len(fits)))]
                acts[b, t, u, labels[b, u]] += gain
                acts[b, t, u, V + i] += gain
                frames[b, u], durs[b, u] = t, durations[i]
                t, u = t + durations[i], u + 1
                continue
            i = blanks[int(rng.integers(len(blanks)))]
            acts[b, t, u, blank] += gain
            acts[b, t, u, V + i] += gain
            t += durations[i]
            if t == T:
                break
    return acts, labels, il, ll, frames[:, :L], durs[:, :L]


def random_case(seed, lengths, V, D, scale=1.0, blank=0):
    """tdt_cases.ragged_case: one utterance per (T_b, L_b)."""
    return tc.ragged_case(lengths, V, D, seed, scale, blank)


# Scripted lattices (the sink trick of tests/align_cases.py, once per softmax): V = 3 tokens -- blank 0, the label 1, a sink 2 at
# logit 0 -- and the duration set [0, 1, 2, 8] on T <= 7 frames, where no edge of duration 8 exists: its logit, 0, is the duration
# sink.  Every other logit is <= -40, so both normalisers are exactly 0 in float32 and float64, every log-probability is the dyadic
# logit itself, every path sum is exact in float64 and ties are exact ties.
SCRIPT_DURATIONS = (0, 1, 2, 8)
SCRIPT_BLANK = 0


def _scripted(lpb, lpl, ld=None):
    """lpb [T, L+1], lpl [T, L] token log-probabilities; ld [T, L+1, 3] duration log-probabilities (default -48 everywhere)."""
    lpb, lpl = np.asarray(lpb, np.float32), np.asarray(lpl, np.float32)
    T, U = lpb.shape
    assert T <= 7 and lpl.shape == (T, U - 1)
    ld = np.full((T, U, 3), -48.0, np.float32) if ld is None else np.asarray(ld, np.float32)
    acts = np.zeros((1, T, U, 3 + 4), np.float32)
    acts[0, :, :, 0] = lpb
    acts[0, :, : U - 1, 1] = lpl
    acts[0, :, U - 1, 1] = -48.0
    acts[0, :, :, 3:6] = ld
    labels = np.ones((1, U - 1), np.int32)
    return acts, labels, np.array([T], np.int32), np.array([U - 1], np.int32)


def scripted_all_tie(T=7, L=5):
    """Every edge weighs -96: the paths with the fewest edges (6) tie and the tie rule alone decides among them."""
    return _scripted(np.full((T, L + 1), -48.0), np.full((T, L), -48.0)), np.array([0, 2, 4, 6, 6]), np.array([2, 2, 2, 0, 0]), -576.0


def scripted_ulp(T=7, L=5, t_star=3, u_star=2):
    """As above, but the label logit of cell (t_star, u_star) is one float32 ulp higher: the best path of the float64 restatement
    must use that edge.  NOT exact in float32: the edge weight (-48 + 2^-18) + -48 lies half way between two float32 numbers and
    the contract's single rounding returns -96, the weight of every other edge -- on float32 weights this lattice is the all-tie
    one again (SCRIPTED_F64_ONLY; scripted_ulp32 is the float32-exact twin)."""
    lpl = np.full((T, L), -48.0, np.float32)
    lpl[t_star, u_star] = np.nextafter(np.float32(-48.0), np.float32(0.0))
    return _scripted(np.full((T, L + 1), -48.0), lpl), np.array([0, 2, 3, 5, 6]), np.array([2, 1, 2, 1, 0]), None


def scripted_ulp32(T=7, L=5, t_star=3, u_star=2):
    """scripted_ulp with token logits of -80 and duration logits of -40: the raised weight, (-80 + 2^-17) + -40, is a float32 number
    (the sum stays in the binade of -80), so the one-ulp preference survives the float32 weights of the engine."""
    lpl = np.full((T, L), -80.0, np.float32)
    lpl[t_star, u_star] = np.nextafter(np.float32(-80.0), np.float32(0.0))
    case = _scripted(np.full((T, L + 1), -80.0), lpl, np.full((T, L + 1, 3), -40.0))
    return case, np.array([0, 2, 3, 5, 6]), np.array([2, 1, 2, 1, 0]), None


def scripted_late(T=7, L=3):
    """Cheap blanks along u = 0 and every label cheap only in the last frame: three blank jumps of 2, then all labels in frame
    T - 1 over duration 0."""
    lpb, lpl = np.full((T, L + 1), -400.0), np.full((T, L), -400.0)
    lpb[:, 0] = -40.0
    lpl[T - 1, :] = -40.0
    return _scripted(lpb, lpl), np.full(L, T - 1), np.zeros(L, np.int64), -976.0


def scripted_early(T=7, L=3):
    """The mirror image: every label cheap only in frame 0, cheap blanks along the last column.  Labels 0 and 1 take duration 0; the
    last one jumps, and the exact ties among its durations and the blank chains behind it (six edges either way) go by the tie
    rule: the terminal keeps its first candidate, the blank of duration 1, and the label ends up with duration 2."""
    lpb, lpl = np.full((T, L + 1), -400.0), np.full((T, L), -400.0)
    lpb[:, L] = -40.0
    lpl[0, :] = -40.0
    return _scripted(lpb, lpl), np.zeros(L, np.int64), np.array([0, 0, 2]), -528.0


SCRIPTED = {"all_tie": scripted_all_tie, "ulp": scripted_ulp, "ulp32": scripted_ulp32, "late": scripted_late, "early": scripted_early}
SCRIPTED_F64_ONLY = ("ulp",)  # exact in float64 alone: see scripted_ulp


def float32_exact(ref):
    """True when every edge weight of a restated utterance is a float32 number: the engine's float32 weights ARE the restatement's."""
    return all((w.astype(np.float32).astype(np.float64) == w).all() for w in (ref["wb"], ref["wl"]))
