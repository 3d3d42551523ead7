"""The beam search with several symbols per frame (include/rnnt_beam_multi.h), for its tests (a helper module, not a conftest).

  MultiRestatement  the rule of the header in float64 on the logits a `logits_fn(b, t, y)` returns, written from the header text;
                    nothing is shared with joint.MultiBeamJoint.  It counts the events the scenarios assert and checks their
                    precondition: adjacent ranked entries are declared ties or more than twice the score bar apart.
  brute_force       log of the sum, over every alignment of a sequence that emits at most E symbols at a frame and then that frame's
                    blank, of the alignment's probability.
  run_multibeam     plays the caller of the header: one token sequence per row (2 K rows per utterance), gathered by `parents`,
                    grown by `emitted`, the script evaluated for the rows of the open list.
  scenarios         scripted logits (tests/decode_scripts.py's ScriptedJoint and scripts) with the events each must show.

Score bar after n steps: decode_scripts.score_bar(n, max |lse|, s) -- a path takes at most one log-softmax per step (round), each
with the logsumexp bar of the step tests; a logaddexp of two scores within the bar stays within it."""
import math
from dataclasses import dataclass, field

import numpy as np

from tests import decode_scripts as ds


# ---------------------------------------------------------------------------------------------
# the rule, restated
# ---------------------------------------------------------------------------------------------
@dataclass
class MultiEvents:
    closed_merges: int = 0      # closings added into an entry the closed list held already
    merges_by_round: dict = field(default_factory=dict)
    open_closed_pairs: int = 0  # (step, sequence) with the sequence in both lists after the step: they must not merge
    overflows: int = 0          # closed lists longer than K before the cut
    ties: int = 0
    empty_turns: list = field(default_factory=list)  # (utterance, frame): the closed list was empty at the frame turn
    capped: int = 0             # open hypotheses of max_hyp_len tokens (they offer no expansion)
    skipped_closings: int = 0   # NaN / -inf closings
    max_candidates: int = 0     # the longest candidate list
    max_closed: int = 0         # the longest closed list before the cut
    max_lse: float = 0.0
    min_gap: float = math.inf


class MultiRestatement:
    def __init__(self, logits_fn, B, K, E, N, frame_lengths, maxT, blank, ties_allowed=False):
        self.fn, self.B, self.K, self.E, self.N, self.blank, self.ties_allowed = logits_fn, B, K, E, N, blank, ties_allowed
        self.Tb = [min(max(int(f), 0), maxT) for f in frame_lengths]
        self.open = [[((), 0.0)] for _ in range(B)]
        self.closed = [[] for _ in range(B)]
        self.k = 0
        self.ev = MultiEvents()

    def _gap(self, hi, lo, what):
        gap = hi - lo
        if gap == 0.0:
            assert self.ties_allowed, f"scenario precondition: unintended exact tie ({what})"
            self.ev.ties += 1
            return
        bar = ds.score_bar(self.k + 1, self.ev.max_lse, max(abs(hi), abs(lo)))
        self.ev.min_gap = min(self.ev.min_gap, gap)
        assert gap > 2 * bar, f"scenario precondition: {gap:.3e} apart, bar {bar:.3e} ({what})"

    def step(self):
        """One round of every utterance -> (parents, emitted) over the B 2K rows, as the library must write them."""
        K, E, blank = self.K, self.E, self.blank
        KR = 2 * K
        t, rnd = divmod(self.k, E + 1)
        parents, emitted = list(range(self.B * KR)), [-1] * (self.B * KR)
        for b in range(self.B):
            if t >= self.Tb[b]:
                continue
            rb = b * KR
            A, Bl = self.open[b], self.closed[b]
            lps = []
            for y, _ in A:  # 1. joint
                lg = np.asarray(self.fn(b, t, y), np.float64)
                lse = ds._logsumexp(lg)
                if math.isfinite(lse):
                    self.ev.max_lse = max(self.ev.max_lse, abs(lse))
                lps.append(lg - lse)
            lst = [[y, s, K + j] for j, (y, s) in enumerate(Bl)]  # 2. closings: [sequence, score, the slot of its state]
            for i, (y, s) in enumerate(A):
                c = s + float(lps[i][blank])
                if c != c or c == -math.inf:
                    self.ev.skipped_closings += 1
                    continue
                for e in lst:
                    if e[0] == y:
                        e[1] = ds._logaddexp(e[1], c)
                        self.ev.closed_merges += 1
                        self.ev.merges_by_round[rnd] = self.ev.merges_by_round.get(rnd, 0) + 1
                        break
                else:
                    lst.append([y, c, i])
            self.ev.max_closed = max(self.ev.max_closed, len(lst))
            self.ev.overflows += len(lst) > K
            lst = [lst[j] for j in sorted(range(len(lst)), key=lambda j: -lst[j][1])]  # (stable)
            for j in range(min(K, len(lst) - 1)):
                self._gap(lst[j][1], lst[j + 1][1], f"utterance {b} frame {t} round {rnd} closed {j}")
            lst = lst[:K]
            if rnd < E:  # 3. expansions
                cands = []
                for i, (y, s) in enumerate(A):
                    if len(y) >= self.N:
                        self.ev.capped += 1
                        continue
                    for v in range(lps[i].shape[0]):
                        sc = s + float(lps[i][v])
                        if v != blank and sc == sc and sc > -math.inf:
                            cands.append((sc, i, v))
                self.ev.max_candidates = max(self.ev.max_candidates, len(cands))
                cands.sort(key=lambda c: (-c[0], c[1], c[2]))
                for j in range(min(K, len(cands) - 1)):
                    self._gap(cands[j][0], cands[j + 1][0], f"utterance {b} frame {t} round {rnd} candidate {j}")
                cands = cands[:K]
                for k, (sc, i, v) in enumerate(cands):
                    parents[rb + k], emitted[rb + k] = rb + i, v
                for k, e in enumerate(lst):
                    parents[rb + K + k] = rb + e[2]
                self.open[b] = [(A[i][0] + (v,), sc) for sc, i, v in cands]
                self.closed[b] = [(e[0], e[1]) for e in lst]
                self.ev.open_closed_pairs += len({y for y, _ in self.open[b]} & {y for y, _ in self.closed[b]})
            else:  # 4. the frame turn
                if not lst:
                    self.ev.empty_turns.append((b, t))
                for k, e in enumerate(lst):
                    parents[rb + k] = rb + e[2]
                self.open[b] = [(e[0], e[1]) for e in lst]
                self.closed[b] = []
        self.k += 1
        return parents, emitted


def brute_force(logits_fn, b, T, E, blank, y):
    """log sum over every alignment of y over T frames: k_t <= E symbols at frame t, then the frame's blank."""
    cache = {}

    def lp(t, prefix):
        if (t, prefix) not in cache:
            lg = np.asarray(logits_fn(b, t, prefix), np.float64)
            cache[(t, prefix)] = lg - ds._logsumexp(lg)
        return cache[(t, prefix)]

    terms = []

    def walk(t, pos, acc):
        if t == T:
            if pos == len(y):
                terms.append(acc)
            return
        a = acc
        for k in range(E + 1):  # k symbols at frame t, then its blank
            walk(t + 1, pos + k, a + float(lp(t, y[: pos + k])[blank]))
            if k == E or pos + k >= len(y):
                break
            a = a + float(lp(t, y[: pos + k])[y[pos + k]])

    walk(0, 0, 0.0)
    return ds._logsumexp(np.asarray(terms)) if terms else -math.inf


# ---------------------------------------------------------------------------------------------
# the caller
# ---------------------------------------------------------------------------------------------
def run_multibeam(engine, sj, script, B, K, E, N, frame_lengths, maxT, blank, steps, logits_fn, ties_allowed=False, check=True):
    """`engine` has begin() / step(rows [B 2K, J]) -> (parents, emitted) / results() -> (hyps [B, K, N], lengths, scores), all
    numpy.  With check, every step and the results are held against the restatement.  -> (trace, restatement, worst score error,
    its bar)."""
    ref = MultiRestatement(logits_fn, B, K, E, N, frame_lengths, maxT, blank, ties_allowed)
    KR = 2 * K
    seqs = [()] * (B * KR)
    trace = []
    engine.begin()
    junk = np.full((sj.V,), -0.37 * sj.c)
    for step in range(steps):
        t = step // (E + 1)
        L = np.empty((B * KR, sj.V))
        for r in range(B * KR):
            b, k = divmod(r, KR)
            live = t < ref.Tb[b] and k < len(ref.open[b])
            L[r] = script(b, t, seqs[r]) if live else junk
        parents, emitted = engine.step(sj.pred_rows(L))
        trace.append((parents.copy(), emitted.copy()))
        seqs = [seqs[p] + ((e,) if e >= 0 else ()) for p, e in zip(parents.tolist(), emitted.tolist())]
        want_p, want_e = ref.step()
        if not check:
            continue
        assert parents.tolist() == want_p, (step, parents.tolist(), want_p)
        assert emitted.tolist() == want_e, (step, emitted.tolist(), want_e)
        for b in range(B):  # the parents / emitted contract: the caller's sequences are the lists'
            for k, (y, _) in enumerate(ref.open[b]):
                assert seqs[b * KR + k] == y, (step, b, k)
            for k, (y, _) in enumerate(ref.closed[b]):
                assert seqs[b * KR + K + k] == y, (step, b, k, "closed")
    hyps, lengths, scores = engine.results()
    trace.append((hyps.copy(), lengths.copy(), scores.copy()))
    worst, worst_bar = 0.0, 0.0
    if check:
        assert hyps.shape == (B, K, N)
        for b in range(B):
            beam = ref.open[b]
            for k in range(K):
                if k < len(beam):
                    y, s = beam[k]
                    assert lengths[b, k] == len(y) and hyps[b, k, : len(y)].tolist() == list(y), (b, k)
                    assert not hyps[b, k, len(y):].any(), (b, k, "zero padding")
                    err, bar = abs(float(scores[b, k]) - s), ds.score_bar(steps, ref.ev.max_lse, s)
                    assert err <= bar, (b, k, float(scores[b, k]), s, err, bar)
                    if err >= worst:
                        worst, worst_bar = err, bar
                else:
                    assert lengths[b, k] == 0 and scores[b, k] == -math.inf and not hyps[b, k].any(), (b, k, "empty slot")
    return trace, ref, worst, worst_bar


# ---------------------------------------------------------------------------------------------
# scripts
# ---------------------------------------------------------------------------------------------
def path_script(seed, V, blank, plan, level=6.0):
    """plan[b][t]: the symbols utterance b is to emit at frame t.  A hypothesis that is on the planned path gets its next symbol
    (or, with the frame's symbols out, the blank) at 0; every other logit is random in (-level - 3, -level], by (frame, length,
    last token): off-path hypotheses prefer nothing much, and no two different paths add up to the same score."""
    def script(b, t, y):
        rows = plan[b]
        target = tuple(v for row in rows for v in row)
        before = sum(len(row) for row in rows[:t])
        here = len(rows[t]) if t < len(rows) else 0
        L = -level - 3.0 * ds._uniform(V, seed, b, t, len(y), y[-1] if y else V)
        if y == target[: len(y)] and before <= len(y) < before + here:
            L[target[len(y)]] = 0.0
        else:
            L[blank] = 0.0
        return L

    return script


def nan_for(script, V, pred):
    """`script`, but a row of NaN where pred(b, t, y)."""
    def wrapped(b, t, y):
        return np.full(V, np.nan) if pred(b, t, y) else script(b, t, y)

    return wrapped


def softmax_script(seed, V):
    """Random log-softmaxes in a narrow range by (utterance, frame, sequence): every path matters (the exactness shapes)."""
    def script(b, t, y):
        x = 1.5 * ds._uniform(V, seed, b, t, len(y), ds.rolling_hash(y, 1000003) % (1 << 31))
        return x - ds._logsumexp(x)

    return script


def seq_script(seed, V, spread, blank, blank_shift=0.0):
    """Random logits in (-spread, 0] by (utterance, frame, whole sequence), the blank moved by blank_shift: no two paths see the
    same rows, so sums of different paths do not coincide."""
    def script(b, t, y):
        L = -spread * ds._uniform(V, seed, b, t, len(y), ds.rolling_hash(y, 1000003) % (1 << 31))
        L[blank] += blank_shift
        return L

    return script


@dataclass
class MultiScenario:
    name: str
    dtype: int
    V: int
    B: int
    K: int
    E: int
    maxT: int
    frames: list
    blank: int
    script: object
    N: int = 0  # max_hyp_len (0: maxT E)
    ties_allowed: bool = False
    expect: dict = field(default_factory=dict)  # lower bounds on MultiEvents counters; "empty_turns": the exact list
    best: dict = field(default_factory=dict)    # utterance -> the sequence its best hypothesis must be

    @property
    def joint(self):
        return ds.ScriptedJoint(64 if self.dtype == 0 else 128, self.V, 16.0, self.dtype)

    @property
    def max_hyp_len(self):
        return self.N or self.maxT * self.E

    @property
    def steps(self):
        return self.maxT * (self.E + 1)


def scenarios():
    """Every scripted scenario, by name.  The seeds were picked on the restatement alone (wide gaps, the events asserted)."""
    out = []
    # two symbols in one frame, then none for two frames
    out.append(MultiScenario("two-then-none", 0, 7, 1, 3, 2, 3, [3], 0, path_script(11, 7, 0, [[[3, 5], [], []]]),
                             best={0: (3, 5)}))
    # more labels than frames: 5 tokens on 2 frames
    out.append(MultiScenario("more-labels-than-frames", 1, 40, 1, 4, 3, 2, [2], 39, path_script(12, 40, 39, [[[7, 1, 30], [2, 9]]]),
                             best={0: (7, 1, 30, 2, 9)}))
    # closed / closed merges across rounds; an open and a closed hypothesis with the same sequence; the closed list beyond K
    out.append(MultiScenario("merges", 0, 6, 3, 4, 2, 5, [5, 3, 7], 0, ds.random_script(1, 6, spread=3.0, blank=0),
                             expect=dict(closed_merges=6, open_closed_pairs=6, overflows=6)))
    out.append(MultiScenario("merges-f16", 1, 100, 2, 3, 3, 4, [4, 4], 99, ds.random_script(12, 100, spread=5.0, blank=99),
                             expect=dict(closed_merges=2, open_closed_pairs=2, overflows=4)))
    # exact ties: candidates by (hypothesis, symbol), closed entries by their place in the list
    out.append(MultiScenario("ties", 0, 9, 3, 4, 2, 5, [5, 6, 3], 0, ds.tie_script(9, 3, 6, 0), ties_allowed=True, expect=dict(ties=8)))
    out.append(MultiScenario("ties-f16", 1, 128, 2, 2, 1, 6, [6, 4], 4, ds.tie_script(128, 5, 40, 4), ties_allowed=True,
                             expect=dict(ties=4)))
    # a NaN row for every hypothesis of utterance 1 at frame 2: nothing closes, the closed list is empty at the turn and the beam
    # stays empty; for one hypothesis alone in utterance 0
    out.append(MultiScenario("nan-rows", 0, 7, 3, 3, 2, 5, [5, 5, 4], 0,
                             nan_for(ds.random_script(1, 7, spread=3.0, blank=0), 7,
                                     lambda b, t, y: (b == 1 and t == 2) or (b == 0 and t == 1 and len(y) == 1)),
                             expect=dict(skipped_closings=2, empty_turns=[(1, 2), (1, 3), (1, 4)])))
    # max_hyp_len reached
    out.append(MultiScenario("full-rows", 0, 5, 2, 3, 2, 4, [4, 4], 4, seq_script(8, 5, 2.0, 4, -3.0), N=3, expect=dict(capped=4)))
    # ragged lengths with a 0, one beyond maxT
    out.append(MultiScenario("ragged", 1, 33, 5, 2, 2, 4, [4, 0, 9, 1, 2], 0, ds.random_script(1, 33, spread=4.0, blank=0)))
    out.append(MultiScenario("beam-1", 0, 8, 2, 1, 3, 4, [4, 3], 7, ds.random_script(1, 8, spread=3.0)))
    out.append(MultiScenario("one-symbol", 0, 8, 2, 5, 1, 5, [5, 4], 0, ds.random_script(1, 8, spread=3.0, blank=0),
                             expect=dict(closed_merges=1)))
    out.append(MultiScenario("eight-symbols", 1, 20, 2, 16, 8, 2, [2, 1], 19, seq_script(3, 20, 2.0, 19)))
    return {sc.name: sc for sc in out}


NAMES = ["two-then-none", "more-labels-than-frames", "merges", "merges-f16", "ties", "ties-f16", "nan-rows", "full-rows", "ragged",
         "beam-1", "one-symbol", "eight-symbols"]
EXACT_SHAPES = [(4, 2, 3), (3, 3, 1), (5, 2, 2)]  # (T, V, E): with beam 16 nothing is pruned


def check_expectations(sc, ref):
    ev = ref.ev
    for key, want in sc.expect.items():
        got = getattr(ev, key)
        if key == "empty_turns":
            assert got == want, (sc.name, key, got, want)
        else:
            assert got >= want, (sc.name, key, got, want)
    for b, y in sc.best.items():
        assert ref.open[b] and ref.open[b][0][0] == tuple(y), (sc.name, b, ref.open[b][:1])


def describe(sc, ref, worst, bar):
    ev = ref.ev
    return (f"{sc.name}: merges={ev.closed_merges} {dict(ev.merges_by_round)} open/closed pairs={ev.open_closed_pairs} "
            f"overflows={ev.overflows} ties={ev.ties} empty turns={ev.empty_turns} capped={ev.capped} skipped={ev.skipped_closings} "
            f"lists <= {ev.max_candidates}/{ev.max_closed} min gap={ev.min_gap:.3e} worst score error={worst:.3e} (bar {bar:.3e})")
