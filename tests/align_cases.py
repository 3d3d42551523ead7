"""Test infrastructure for forced alignment: the float64 NumPy restatement of the definition in include/rnnt.h (a dense
max-plus recurrence with the tie rule, a back-trace, a scorer for any given path, a brute-force maximum for tiny lattices) and
the input builders the CPU and GPU tests share (random, planted and scripted lattices).  Nothing here touches the engine."""
from __future__ import annotations

import itertools

import numpy as np

from oracle.rnnt_oracle import _gather, log_softmax

NEG = -np.inf


# ---- the restatement --------------------------------------------------------------------------------------------------
def cell_logprobs(acts_b, labels_b, T_b, U_b, blank):
    """acts_b [T, U, V] -> (lpb [T_b, U_b+1], lpl [T_b, U_b]) in float64, from the float64 log-softmax of the logits."""
    lp = log_softmax(np.asarray(acts_b)[:T_b, : U_b + 1])
    return _gather(lp, np.asarray(labels_b)[:U_b], blank)


def viterbi(lpb, lpl):
    """Dense recurrence.  Returns (v [T, U1], took_label [T, U1] bool, margin [T, U1]): margin is |blank arrival - label arrival|
    for cells with two predecessors and +inf elsewhere.  Tie rule: the label arrival wins only if strictly greater."""
    T, U1 = lpb.shape
    v = np.full((T, U1), NEG)
    took = np.zeros((T, U1), dtype=bool)
    margin = np.full((T, U1), np.inf)
    v[0, 0] = 0.0
    for t in range(T):
        for u in range(U1):
            if t == 0 and u == 0:
                continue
            a = v[t - 1, u] + lpb[t - 1, u] if t > 0 else NEG
            c = v[t, u - 1] + lpl[t, u - 1] if u > 0 else NEG
            took[t, u] = c > a
            v[t, u] = c if c > a else a
            if t > 0 and u > 0:
                margin[t, u] = abs(a - c)
    return v, took, margin


def backtrace(took):
    """-> (frames [U], cells on the path as (t, u), last cell first)."""
    T, U1 = took.shape
    t, u = T - 1, U1 - 1
    frames = np.full(U1 - 1, -1, dtype=np.int64)
    cells = [(t, u)]
    while t > 0 or u > 0:
        if took[t, u]:
            u -= 1
            frames[u] = t
        else:
            t -= 1
        cells.append((t, u))
    return frames, cells


def score_path(lpb, lpl, frames):
    """Float64 log-probability of the path that emits label u in frame frames[u] (non-decreasing, within [0, T))."""
    T, U1 = lpb.shape
    frames = [int(f) for f in frames]
    assert len(frames) == U1 - 1
    total, t = 0.0, 0
    for u, f in enumerate(frames):
        assert t <= f < T, (frames, T)
        total += float(lpb[t:f, u].sum()) if f > t else 0.0
        total += float(lpl[f, u])
        t = f
    total += float(lpb[t:T, U1 - 1].sum())
    return total


def brute_force_best(lpb, lpl):
    """max over all C(T+U-1, U) monotone paths."""
    T, U1 = lpb.shape
    return max(score_path(lpb, lpl, fr) for fr in itertools.combinations_with_replacement(range(T), U1 - 1))


def restate(acts_b, labels_b, T_b, U_b, blank=0):
    """One utterance: dict(frames, score, logp, min_margin, lpb, lpl) of the restatement's best path."""
    lpb, lpl = cell_logprobs(acts_b, labels_b, T_b, U_b, blank)
    v, took, margin = viterbi(lpb, lpl)
    frames, cells = backtrace(took)
    score = v[T_b - 1, U_b] + lpb[T_b - 1, U_b]
    mm = min([margin[t, u] for t, u in cells] + [np.inf])
    logp = np.array([lpl[f, u] for u, f in enumerate(frames)])
    return dict(frames=frames, score=float(score), logp=logp, min_margin=float(mm), lpb=lpb, lpl=lpl)


def check_valid_path(frames_row, T_b, U_b):
    """The validity conditions of the issue for one utterance's token_frames row (padded with -1)."""
    fr = np.asarray(frames_row)
    assert (fr[:U_b] >= 0).all() and (fr[:U_b] < T_b).all(), (fr, T_b, U_b)
    assert (fr[U_b:] == -1).all(), (fr, U_b)
    assert int((fr >= 0).sum()) == U_b
    assert (np.diff(fr[:U_b]) >= 0).all(), fr


# ---- inputs -----------------------------------------------------------------------------------------------------------
def random_case(rng, B, T, U, V, scale=1.0, ragged=True, blank=0):
    acts = (scale * rng.normal(size=(B, T, U, V))).astype(np.float32)
    r = rng.integers(0, V - 1, size=(B, max(U - 1, 0)))
    labels = (r + (r >= blank)).astype(np.int32)  # any symbol but the blank
    if ragged:
        il = rng.integers(max(1, T // 2), T + 1, size=B).astype(np.int32)
        ll = rng.integers(0, U, size=B).astype(np.int32)
        il[0], ll[0] = T, U - 1
    else:
        il, ll = np.full(B, T, np.int32), np.full(B, U - 1, np.int32)
    return acts, labels, il, ll


def planted_case(rng, B, T, U, V, gain, late_every=2, ragged=True):
    """N(0,1) logits plus `gain` on one symbol per cell: blank until the cell's label is due, the label afterwards (the kind of
    posteriors train.synthetic_trained_like_joint builds); every late_every-th utterance emits in its last 40 % of frames.
    Returns (acts, labels, il, ll, emit [B, U-1] planted frames, -1 past L_b)."""
    acts = rng.normal(size=(B, T, U, V)).astype(np.float32)
    labels = rng.integers(1, V, size=(B, U - 1)).astype(np.int32)
    if ragged:
        il = rng.integers(max(2, T // 2), T + 1, size=B).astype(np.int32)
        ll = rng.integers((U - 1) // 2, U, size=B).astype(np.int32)
        il[0], ll[0] = T, U - 1
    else:
        il, ll = np.full(B, T, np.int32), np.full(B, U - 1, np.int32)
    emit = np.full((B, U - 1), -1, dtype=np.int64)
    for b in range(B):
        Tb, Lb = int(il[b]), int(ll[b])
        lo = int(0.6 * Tb) if (late_every and b % late_every == late_every - 1) else 0
        e = np.sort(rng.integers(lo, max(Tb, lo + 1), size=Lb))
        emit[b, :Lb] = e
        for u in range(Lb + 1):
            due = e[u] if u < Lb else Tb  # the last column only ever emits blanks
            acts[b, :due, u, 0] += gain
            if u < Lb:
                acts[b, due:, u, labels[b, u]] += gain
    return acts, labels, il, ll, emit


# Scripted lattices: a third "sink" symbol with logit 0 carries all the mass, blank and label logits are dyadic values below -40,
# so log-softmax returns them EXACTLY in float32 and float64 (the normaliser is log(1 + 2 e^-40...) = 0 in both) and every path
# sum is exact in float64: ties are exact ties.
SINK_V, SINK_BLANK, SINK_LABEL = 3, 0, 1


def _scripted(lpb, lpl):
    T, U1 = lpb.shape
    acts = np.zeros((1, T, U1, SINK_V), dtype=np.float32)
    acts[0, :, :, SINK_BLANK] = lpb
    acts[0, :, :, SINK_LABEL] = -64.0
    acts[0, :, : U1 - 1, SINK_LABEL] = lpl
    labels = np.full((1, U1 - 1), SINK_LABEL, dtype=np.int32)
    return acts, labels, np.array([T], np.int32), np.array([U1 - 1], np.int32)


def scripted_all_tie(T=9, U1=6):
    """Every path has the same value: the tie rule alone decides -- blank arrivals everywhere, so every label is emitted in frame 0."""
    case = _scripted(np.full((T, U1), -48.0), np.full((T, U1 - 1), -48.0))
    return case, np.zeros(U1 - 1, dtype=np.int64)


def scripted_ulp(T=9, U1=6, t_star=5, u_star=2):
    """As above, but the label out of (t_star, u_star) is one float32 ulp more probable: the best path must use that edge, i.e.
    emit label u_star in frame t_star; before it the tie rule puts labels 0 ... u_star-1 in frame 0, after it the later labels
    in frame t_star too (blank arrivals on ties, walking back from the last cell)."""
    lpl = np.full((T, U1 - 1), -48.0, dtype=np.float32)
    lpl[t_star, u_star] = np.nextafter(np.float32(-48.0), np.float32(0.0))
    case = _scripted(np.full((T, U1), -48.0, dtype=np.float32), lpl)
    expect = np.array([0] * u_star + [t_star] * (U1 - 1 - u_star), dtype=np.int64)
    return case, expect


def scripted_late(T=9, U1=6):
    """Cheap blanks along u = 0 and cheap labels in the last frame: everything is emitted in frame T - 1."""
    lpb, lpl = np.full((T, U1), -64.0), np.full((T, U1 - 1), -64.0)
    lpb[:, 0] = -40.0
    lpl[T - 1, :] = -40.0
    return _scripted(lpb, lpl), np.full(U1 - 1, T - 1, dtype=np.int64)


def scripted_early(T=9, U1=6):
    """The mirror image: cheap labels in frame 0 and cheap blanks along the last column."""
    lpb, lpl = np.full((T, U1), -64.0), np.full((T, U1 - 1), -64.0)
    lpb[:, U1 - 1] = -40.0
    lpl[0, :] = -40.0
    return _scripted(lpb, lpl), np.zeros(U1 - 1, dtype=np.int64)


SCRIPTED = {"all_tie": scripted_all_tie, "ulp": scripted_ulp, "late": scripted_late, "early": scripted_early}
