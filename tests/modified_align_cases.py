"""Test infrastructure for forced alignment on the modified (one symbol per frame) lattice: the float64 NumPy restatement of the
definition in include/rnnt_modified_align.h (a dense max-plus recurrence over the nodes (t, u), 0 <= t <= T, with the tie rule and
the margins of its decisions, a back-trace, a scorer for any strictly increasing frame list, a brute-force maximum for tiny
lattices) and the input builders the CPU and GPU tests share.  Random and scripted inputs reuse the builders of
tests/align_cases.py; the planted builder here draws its emission frames WITHOUT replacement, one label per frame at most.
Nothing here touches the engine."""
from __future__ import annotations

import itertools

import numpy as np

from tests import align_cases as ac

NEG = -np.inf
cell_logprobs = ac.cell_logprobs  # acts_b [T, U, V] -> (lpb [T_b, L_b+1], lpl [T_b, L_b]) from the float64 log-softmax
random_case = ac.random_case
SINK_BLANK = ac.SINK_BLANK


# ---- the restatement --------------------------------------------------------------------------------------------------
def viterbi(lpb, lpl):
    """Dense recurrence over the nodes.  Returns (v [T+1, L+1], took_label [T+1, L+1] bool, margin [T+1, L+1]): margin is
    |blank arrival - label arrival| for nodes with two reachable predecessors and +inf elsewhere.  Tie rule: the label arrival
    wins only if strictly greater.  (No band is needed here: a node a path cannot pass through is either -inf or never met by
    the back-trace from (T, L).)"""
    T, U1 = lpb.shape
    v = np.full((T + 1, U1), NEG)
    took = np.zeros((T + 1, U1), dtype=bool)
    margin = np.full((T + 1, U1), np.inf)
    v[0, 0] = 0.0
    for t in range(1, T + 1):  # (a row at a time: the same elementwise float64 operations as a loop over u)
        a = v[t - 1] + lpb[t - 1]
        c = np.concatenate([[NEG], v[t - 1, : U1 - 1] + lpl[t - 1]])
        took[t] = c > a
        v[t] = np.where(took[t], c, a)
        both = (a > NEG) & (c > NEG)
        margin[t, both] = np.abs(a[both] - c[both])
    return v, took, margin


def backtrace(took):
    """One step per frame from (T, L) -> (frames [L], the nodes on the path as (t, u), last node first)."""
    T, L = took.shape[0] - 1, took.shape[1] - 1
    u = L
    frames = np.full(L, -1, dtype=np.int64)
    nodes = [(T, u)]
    for t in range(T, 0, -1):
        if took[t, u]:
            u -= 1
            frames[u] = t - 1
        nodes.append((t - 1, u))
    assert u == 0, (u, frames)
    return frames, nodes


def score_path(lpb, lpl, frames):
    """Float64 log-probability of the path that emits label u in frame frames[u] (STRICTLY increasing, within [0, T)) and a blank
    in every other frame."""
    T, U1 = lpb.shape
    frames = [int(f) for f in frames]
    assert len(frames) == U1 - 1
    assert all(0 <= f < T for f in frames) and all(a < b for a, b in zip(frames, frames[1:])), (frames, T)
    total, u = 0.0, 0
    for t in range(T):
        if u < U1 - 1 and frames[u] == t:
            total += float(lpl[t, u])
            u += 1
        else:
            total += float(lpb[t, u])
    assert u == U1 - 1
    return total


def brute_force_best(lpb, lpl):
    """max over all C(T, L) paths: a path picks the L frames that emit a label."""
    T, U1 = lpb.shape
    return max(score_path(lpb, lpl, fr) for fr in itertools.combinations(range(T), U1 - 1))


def restate(acts_b, labels_b, T_b, L_b, blank=0):
    """One utterance: dict(frames, score, logp, min_margin, lpb, lpl) of the restatement's best path.  L_b > T_b: no path --
    score -inf, frames -1, logp 0."""
    lpb, lpl = cell_logprobs(acts_b, labels_b, T_b, L_b, blank)
    if L_b > T_b:
        return dict(frames=np.full(L_b, -1, dtype=np.int64), score=NEG, logp=np.zeros(L_b), min_margin=np.inf, lpb=lpb, lpl=lpl)
    v, took, margin = viterbi(lpb, lpl)
    frames, nodes = backtrace(took)
    mm = min([margin[t, u] for t, u in nodes] + [np.inf])
    logp = np.array([lpl[f, u] for u, f in enumerate(frames)])
    return dict(frames=frames, score=float(v[T_b, L_b]), logp=logp, min_margin=float(mm), lpb=lpb, lpl=lpl)


def check_valid_path(frames_row, T_b, L_b):
    """One utterance's token_frames row (padded with -1): within [0, T), strictly increasing, -1 past L."""
    fr = np.asarray(frames_row)
    assert (fr[:L_b] >= 0).all() and (fr[:L_b] < T_b).all(), (fr, T_b, L_b)
    assert (fr[L_b:] == -1).all(), (fr, L_b)
    assert (np.diff(fr[:L_b]) > 0).all(), fr


# ---- inputs -----------------------------------------------------------------------------------------------------------
def planted_case(rng, B, T, U, V, gain, late_every=2, ragged=True):
    """N(0,1) logits plus `gain` on one symbol per cell: in column u the blank until the frame that emits label u, the label
    from there on; the last column only ever emits blanks.  The emission frames are drawn WITHOUT replacement (one label per
    frame at most, L_b <= T_b); every late_every-th utterance emits in its last 40 % of frames.
    Returns (acts, labels, il, ll, emit [B, U-1] planted frames, -1 past L_b)."""
    assert U - 1 <= T
    acts = rng.normal(size=(B, T, U, V)).astype(np.float32)
    labels = rng.integers(1, V, size=(B, U - 1)).astype(np.int32)
    if ragged:
        ll = rng.integers((U - 1) // 2, U, size=B).astype(np.int32)
        il = np.array([rng.integers(max(2, T // 2, int(l)), T + 1) for l in ll], dtype=np.int32)
        il[0], ll[0] = T, U - 1
    else:
        il, ll = np.full(B, T, np.int32), np.full(B, U - 1, np.int32)
    emit = np.full((B, U - 1), -1, dtype=np.int64)
    for b in range(B):
        Tb, Lb = int(il[b]), int(ll[b])
        lo = int(0.6 * Tb) if (late_every and b % late_every == late_every - 1) else 0
        lo = min(lo, Tb - Lb)
        e = lo + np.sort(rng.choice(Tb - lo, size=Lb, replace=False))
        emit[b, :Lb] = e
        for u in range(Lb + 1):
            due = e[u] if u < Lb else Tb
            acts[b, :due, u, 0] += gain
            if u < Lb:
                acts[b, due:, u, labels[b, u]] += gain
    return acts, labels, il, ll, emit


# Scripted lattices (the sink-symbol trick of tests/align_cases.py): blank and label log-probabilities are dyadic values that
# log-softmax returns EXACTLY in float32 and float64, every path sum is exact in float64, ties are exact ties.
def scripted_all_tie(T=9, U1=6):
    """Every path has the same value: the tie rule alone decides.  Walking back from (T, L) every tie takes the blank arrival, so
    the labels sit where a node has the label arrival only, u = t: frames 0, 1, ... L-1."""
    case = ac._scripted(np.full((T, U1), -48.0), np.full((T, U1 - 1), -48.0))
    return case, np.arange(U1 - 1, dtype=np.int64)


def scripted_ulp(T=9, U1=6, t_star=5, u_star=2):
    """As above, but the label edge out of (t_star, u_star) is one float32 ulp more probable: the best path must use it.  Before
    it the tie rule packs labels 0 ... u_star-1 into frames 0 ... u_star-1; after it the later labels follow in the very next
    frames (walking back from (T, L) blanks are taken until only the chain of label arrivals from (t_star+1, u_star+1) is left)."""
    lpl = np.full((T, U1 - 1), -48.0, dtype=np.float32)
    lpl[t_star, u_star] = np.nextafter(np.float32(-48.0), np.float32(0.0))
    case = ac._scripted(np.full((T, U1), -48.0, dtype=np.float32), lpl)
    expect = np.array(list(range(u_star)) + [t_star + i for i in range(U1 - 1 - u_star)], dtype=np.int64)
    return case, expect


def scripted_late(T=9, U1=6):
    """Cheap blanks along u = 0 and label u cheap only in frame T - L + u: everything is emitted in the last L frames."""
    L = U1 - 1
    lpb, lpl = np.full((T, U1), -64.0), np.full((T, L), -64.0)
    lpb[:, 0] = -40.0
    for u in range(L):
        lpl[T - L + u, u] = -40.0
    return ac._scripted(lpb, lpl), np.arange(T - L, T, dtype=np.int64)


def scripted_early(T=9, U1=6):
    """The mirror image: label u cheap only in frame u, cheap blanks along the last column."""
    L = U1 - 1
    lpb, lpl = np.full((T, U1), -64.0), np.full((T, L), -64.0)
    lpb[:, L] = -40.0
    for u in range(L):
        lpl[u, u] = -40.0
    return ac._scripted(lpb, lpl), np.arange(L, dtype=np.int64)


SCRIPTED = {"all_tie": scripted_all_tie, "ulp": scripted_ulp, "late": scripted_late, "early": scripted_early}
