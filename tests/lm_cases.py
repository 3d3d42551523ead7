"""N-gram LM shallow fusion: restatements and scenarios shared by the CPU and GPU tests (a helper module, not a conftest).

  brute force     BruteLM: log P(v | history) straight from the n-gram dictionary by the textbook back-off recursion (listed:
                  its log-probability; else the back-off weight of the history, where listed, plus the same question for the
                  history without its first token; at the empty history the unknown-token score).  No states.
  array_delta     the transition of include/rnnt_lm.h on the ten fields of rnntLmGraph, arcs found by linear scan, np.float32
                  additions in the header's order.  array_hops: how many hops that walk took and whether it ended in an arc.
  restatement     LmBeamRestatement: rules 2' and 3' in float64 with the f32 key (bias_cases.BiasedBeamRestatement, the row of a
                  state from array_delta here).  Every hypothesis starts in state 0.
  run_lm          the caller of compute_rnnt_beam_*_step_lm (bias_cases.run_biased with the LM restatement): ids, lengths,
                  parents, emitted and lm_states exactly at every step, scores within ds.score_bar with |s| including the LM.

All scripted scores are dyadic (multiples of 1/16, natural logarithms, scale 1), so sums are exact in f32 and float64.  Every
scenario's gaps are asserted on the restatement alone: adjacent keys around the per-hypothesis cut and adjacent ranked candidates
are declared ties or more than twice the bar apart.
"""
import math
from dataclasses import dataclass, field

import numpy as np

from tests import bias_cases as bc
from tests import decode_scripts as ds

BOS, EOS = "<s>", "</s>"


# ---------------------------------------------------------------------------------------------
# the LM, by brute force
# ---------------------------------------------------------------------------------------------
class BruteLM:
    """ngrams {n-gram: (logp, bow)}; scores are mult * value (+ bonus on tokens), float64."""

    def __init__(self, ngrams, mult=1.0, bonus=0.0, unk=-10.0):
        self.t = {tuple(g): (v if isinstance(v, (tuple, list)) else (v, 0.0)) for g, v in ngrams.items()}
        self.mult, self.bonus, self.unk = mult, bonus, unk
        self.has_eos = any(g[-1] == EOS for g in self.t)

    def cond(self, h, w):
        """scaled log P(w | h): h a tuple that starts with BOS"""
        extra = 0.0 if w == EOS else self.bonus
        if h + (w,) in self.t:
            return self.mult * self.t[h + (w,)][0] + extra
        if not h:
            return self.mult * self.unk + extra
        return (self.mult * self.t[h][1] if h in self.t else 0.0) + self.cond(h[1:], w)

    def sentence(self, tokens, eos=True):
        h, total = (BOS,), 0.0
        for v in tokens:
            total += self.cond(h, v)
            h = h + (v,)
        return total + (self.cond(h, EOS) if eos and self.has_eos else 0.0)


def array_delta(g, s, v, blank, hops=False):
    """include/rnnt_lm.h delta(s, v) on the ten fields of g -> (next, beta f32) [, hops taken, ended in an arc]."""
    f32 = np.float32
    if v == blank:
        return (s, f32(0.0), 0, False) if hops else (s, f32(0.0))
    E, cur, hop, acc = int(g.empty_state), s, 0, f32(0.0)
    while True:
        lo, hi = int(g.arc_offsets[cur]), int(g.arc_offsets[cur + 1])
        hit = np.nonzero(g.arc_tokens[lo:hi] == v)[0]  # (a linear scan: no bisection, no order assumed)
        arc = lo + int(hit[0]) if hit.size else -1
        if arc >= 0:
            beta = f32(g.arc_score[arc]) if hop == 0 else f32(acc + f32(g.arc_score[arc]))
            return (int(g.arc_next[arc]), beta, hop, True) if hops else (int(g.arc_next[arc]), beta)
        if cur == E:
            beta = f32(g.unk_score) if hop == 0 else f32(acc + f32(g.unk_score))
            return (E, beta, hop, False) if hops else (E, beta)
        acc = f32(g.backoff_score[cur]) if hop == 0 else f32(acc + f32(g.backoff_score[cur]))
        cur, hop = int(g.backoff_next[cur]), hop + 1
        if hop == 8:
            cur = E


def random_ngrams(rng, V, blank, order, bos=True, eos=True, grams_per_order=14, dyadic=True):
    """A prefix-closed random table of the given order over the non-blank tokens: log-probabilities in [-4, 0], back-off weights of
    either sign in [-1, 1] (a third of them 0), multiples of 1/8 when dyadic."""
    syms = [v for v in range(V) if v != blank]
    val = (lambda lo, hi: float(rng.integers(int(lo * 8), int(hi * 8) + 1)) / 8) if dyadic else (lambda lo, hi: float(rng.uniform(lo, hi)))
    bow = lambda: 0.0 if rng.integers(0, 3) == 0 else val(-1.0, 1.0)  # noqa: E731
    grams = {}
    for v in syms:
        if rng.integers(0, 4):  # (a quarter of the tokens are unknown to the unigrams)
            grams[(v,)] = (val(-4.0, 0.0), bow())
    if bos:
        grams[(BOS,)] = (-99.0, bow())
    if eos:
        grams[(EOS,)] = (val(-4.0, 0.0), 0.0)
    level = list(grams)
    for n in range(2, order + 1):
        new = []
        heads = [g for g in level if g[-1] != EOS]
        for _ in range(grams_per_order if heads else 0):
            h = heads[int(rng.integers(0, len(heads)))]
            w = EOS if eos and rng.integers(0, 6) == 0 else int(rng.choice(syms))
            if h + (w,) not in grams:
                grams[h + (w,)] = (val(-4.0, 0.0), bow() if n < order and w != EOS else 0.0)
                new.append(h + (w,))
        level = new
    return grams


# ---------------------------------------------------------------------------------------------
# rules 2' and 3' with the LM's transition
# ---------------------------------------------------------------------------------------------
class LmBeamRestatement(bc.BiasedBeamRestatement):
    """bias_cases.BiasedBeamRestatement (float64 scores, the f32 key) with beta and the next state from array_delta above.  A
    beam entry is (y, s, q); q = 0, the sentence start, at begin."""

    def _row(self, q, V):
        if q not in self._rows:
            d = [array_delta(self.g, q, v, self.blank) for v in range(V)]
            self._rows[q] = (np.array([x[1] for x in d], np.float32), [x[0] for x in d])
        return self._rows[q]


def run_lm(engine, sj, script, g, B, K, frame_lengths, maxT, blank, steps, logits_fn, ties_allowed=False):
    """`engine`: begin() / step(rows [B K, J]) -> (parents, emitted, lm_states) / results() -> (hyps, lengths, scores) -- the
    beam's own scores, not finalised.  -> (trace, restatement, worst score error, its bar)."""
    ref = LmBeamRestatement(logits_fn, g, B, K, frame_lengths, maxT, blank, ties_allowed)
    seqs = [()] * (B * K)
    trace = []
    engine.begin()
    junk = np.full((sj.V,), -0.37 * sj.c)
    for step in range(steps):
        L = np.empty((B * K, sj.V))
        for r in range(B * K):
            b, k = divmod(r, K)
            live = step < ref.Tb[b] and k < len(ref.beams[b])
            L[r] = script(b, step, seqs[r]) if live else junk
        parents, emitted, states = engine.step(sj.pred_rows(L))
        trace.append((parents.copy(), emitted.copy(), states.copy()))
        seqs = [seqs[p] + ((e,) if e >= 0 else ()) for p, e in zip(parents.tolist(), emitted.tolist())]
        want_p, want_e, want_q = ref.step()
        assert parents.tolist() == want_p, (step, parents.tolist(), want_p)
        assert emitted.tolist() == want_e, (step, emitted.tolist(), want_e)
        assert states.tolist() == want_q, (step, states.tolist(), want_q)
        for b in range(B):
            for k, e in enumerate(ref.beams[b]):
                assert seqs[b * K + k] == e[0], (step, b, k)
    hyps, lengths, scores = engine.results()
    trace.append((hyps.copy(), lengths.copy(), scores.copy()))
    worst, worst_bar = 0.0, 0.0
    for b in range(B):
        beam = ref.beams[b]
        n = min(steps, ref.Tb[b])
        for k in range(K):
            if k < len(beam):
                y, s, _ = beam[k]
                assert lengths[b, k] == len(y) and hyps[b, k, : len(y)].tolist() == list(y), (b, k)
                assert not hyps[b, k, len(y):].any(), (b, k, "zero padding")
                err, bar = abs(float(scores[b, k]) - s), ds.score_bar(n, ref.ev.max_lse, s)
                print(f"  score b={b} k={k}: got {float(scores[b, k]):.9g} want {s:.9g} error {err:.3e} bar {bar:.3e}")
                assert err <= bar, (b, k, float(scores[b, k]), s, err, bar)
                if err >= worst:
                    worst, worst_bar = err, bar
            else:
                assert lengths[b, k] == 0 and scores[b, k] == -math.inf and not hyps[b, k].any(), (b, k, "empty slot")
    return trace, ref, worst, worst_bar


# ---------------------------------------------------------------------------------------------
# scenarios
# ---------------------------------------------------------------------------------------------
@dataclass
class LmScenario:
    name: str
    dtype: int
    V: int
    B: int
    K: int
    maxT: int
    frames: list
    blank: int
    script: object
    steps: int
    ngrams: dict
    unk: float = -8.0
    J: int = 0  # 0: the scripted joint's default for the dtype; 704 with dtype 0: the wide f32-grade step
    ties_allowed: bool = False
    expect: dict = field(default_factory=dict)

    @property
    def joint(self):
        return ds.ScriptedJoint(self.J or (64 if self.dtype == 0 else 128), self.V, 16.0, self.dtype)


def build_lm(sc, **kw):
    from rnnt_speech_recognition_amd.lm import NgramLM

    return NgramLM.from_ngrams(sc.ngrams, sc.blank, sc.V, unk=sc.unk, log10=False, **kw)


def _unigrams(V, blank, lp):
    return {(v,): (lp, 0.0) for v in range(V) if v != blank}


def flip_scenario(dtype=0, J=0):
    """bias_cases.path_script: paths 1 3 5 (the model's favourite) and 2 4 6, 0.75 behind at frame 0.  The LM knows <s> 2, 2 4 and
    4 6 at -0.5 and everything else as a unigram at -2: 2 4 6 collects -1.5, 1 3 5 collects -6, and the winner flips."""
    V = 9 if dtype == 0 else 70
    grams = _unigrams(V, 0, -2.0)
    grams.update({(BOS,): (-99.0, 0.0), (BOS, 2): (-0.5, 0.0), (2, 4): (-0.5, 0.0), (4, 6): (-0.5, 0.0)})
    return LmScenario("lm-flip", dtype, V, 2, 2, 4, [4, 3], 0, bc.path_script(V, 0, [(1, 3, 5), (2, 4, 6)]), 4, grams, J=J)


DEPTH_PATH = (1, 2, 3, 4, 5, 6, 7)
DEPTH_OFFERS = {1: 0, 9: 1, 10: 2, 11: 4, 3: 8, 8: 8}  # token offered after the path -> the hops its walk takes (8: unknown, at E)


def depth_scenario():
    """An order-9 sparse LM over V = 12: every window of <s> 1 2 3 4 5 6 7, so that the state after the path has a chain of 8
    hops, and continuations listed at one level each: 1 after the whole path (hop 0), 9 after 1 ... 7 (hop 1), 10 after 2 ... 7
    (hop 2), 11 after 4 ... 7 (hop 4); 3 is found as a unigram (hop 8) and 8 nowhere (hop 8, the unknown-token score).  The
    back-off weights alternate in sign.  The hypothesis that has followed the path offers exactly those six tokens at frame 7."""
    V, blank, K = 12, 0, 6
    seq = (BOS,) + DEPTH_PATH
    grams = {}
    for i in range(len(seq)):
        for j in range(i + 1, len(seq) + 1):
            w = seq[i:j]
            grams[w] = (-0.125 * (1 + (i + j) % 2), (0.125 if (i + j) % 2 else -0.25) * (1 + i % 3))
    grams[(BOS,)] = (-99.0, 0.375)
    grams[seq + (1,)] = (-0.5, 0.0)
    grams[seq[1:] + (9,)] = (-0.75, 0.0)
    grams[seq[2:] + (10,)] = (-1.0, 0.0)
    grams[seq[4:] + (11,)] = (-0.625, 0.0)
    offers = list(DEPTH_OFFERS)

    def script(b, t, y):
        L = -9.0 - 5.0 * np.arange(V) / V - 0.013 * t
        y = tuple(y)
        if t < len(DEPTH_PATH) and y == DEPTH_PATH[:t]:
            L[blank], L[DEPTH_PATH[t]] = -12.5 - 0.41 * t, 0.0
        elif t == len(DEPTH_PATH) and y == DEPTH_PATH:
            L[blank] = -14.0
            for n, v in enumerate(offers):
                L[v] = -0.3125 * n
        else:
            L[blank] = 0.0
        return L

    return LmScenario("lm-depth", 0, V, 2, K, 8, [8, 5], blank, script, 8, grams, unk=-2.0)


def positive_backoff_scenario(dtype=0):
    """Paths 1 3 5 and 2 4 6.  1 2 is listed, so 1 is a state; its back-off weight is +1.5: 3 after 1 collects +1.5 - 1 > 0."""
    V = 9 if dtype == 0 else 70
    grams = _unigrams(V, 0, -1.0)
    grams.update({(BOS,): (-99.0, 0.25), (1,): (-1.0, 1.5), (1, 2): (-0.25, 0.0)})
    return LmScenario("lm-positive-backoff", dtype, V, 1, 2, 4, [4], 0, bc.path_script(V, 0, [(1, 3, 5), (2, 4, 6)]), 4, grams)


def tie_scenario(K):
    """ds.tie_script: symbols p and q tie at the top (the LM scores both alike: equal keys, the lower symbol first), then two
    hypotheses with equal scores and equal LM scores tie (hypothesis, then symbol, ascending)."""
    base = ds.tie_scenario(K)
    p, q = (5, 40) if base.dtype == 1 else (3, 6)
    grams = {(p,): (-0.3125, 0.0), (q,): (-0.3125, 0.0), (BOS,): (-99.0, -0.1875)}  # (sixteenths: no tie the script does not make)
    return LmScenario(f"lm-ties-K{K}", base.dtype, base.V, base.B, K, base.maxT, base.frames, base.blank, base.script, base.steps,
                      grams, unk=-1.0, ties_allowed=True, expect=dict(ties=4))


def merge_scenario(K):
    """ds.merge_script (y + x arrives by emission from y and by blank from y + x) under an LM over its symbols."""
    base = ds.merge_scenario(K)
    xs = (base.V - 3, base.V - 2) if base.blank == base.V - 1 else (base.V - 2, base.V - 1)
    grams = {}
    for n, p in enumerate([(1, xs[0]), (2, xs[1], xs[0]), (xs[0], xs[1]), (3,), (xs[1], xs[0], xs[1], xs[0]), (BOS, 1), (BOS, xs[0], xs[1])]):
        for k in range(1, len(p) + 1):
            grams.setdefault(p[:k], (-0.125 * (1 + (n + k) % 5), 0.0 if k == len(p) else 0.125 * ((n + 2 * k) % 4 - 1)))
    return LmScenario(f"lm-merges-K{K}", base.dtype, base.V, base.B, K, base.maxT, base.frames, base.blank, base.script, base.steps,
                      grams, unk=-1.5, expect=dict(merges=4))


def random_scenario(K, B, seed, dtype, nan_at=None):
    """ds.random_script under a random order-4 LM: beam 1 / 4 / 16, B K > 32 rows, ragged frame_lengths with T_b = 0."""
    V, T = (24, 7) if dtype == 0 else (100, 6)
    rng = np.random.default_rng(seed)
    grams = random_ngrams(rng, V, 0, 4, grams_per_order=40)
    frames = [(T, 0, T + 3, T - 2, 3)[b % 5] for b in range(B)]
    return LmScenario(f"lm-random-K{K}-B{B}", dtype, V, B, K, T, frames, 0,
                      ds.random_script(seed, V, spread=4.0, nan_at=nan_at, blank=0), T, grams, unk=-3.0,
                      expect=dict(carried=[nan_at]) if nan_at else {})


def finalise_scenario():
    """Two hypotheses, 5 6 (the model's favourite) and 1 2, level under the LM's token scores; </s> is likely after 2 (-0.25)
    and unlikely after 6 (-4): the end-of-sentence score changes the rank."""
    V = 9
    grams = _unigrams(V, 0, -1.0)
    grams.update({(BOS,): (-99.0, 0.0), (EOS,): (-2.0, 0.0), (2,): (-1.0, 0.0), (6,): (-1.0, 0.0), (2, EOS): (-0.25, 0.0),
                  (6, EOS): (-4.0, 0.0)})
    return LmScenario("lm-finalise", 0, V, 1, 2, 2, [2], 0, bc.path_script(V, 0, [(5, 6), (1, 2)]), 2, grams)


SCENARIOS = {
    "flip0": lambda: flip_scenario(0), "flip1": lambda: flip_scenario(1), "flip2": lambda: flip_scenario(0, J=704),
    "depth": depth_scenario,
    "posbow0": lambda: positive_backoff_scenario(0), "posbow1": lambda: positive_backoff_scenario(1),
    "ties2": lambda: tie_scenario(2), "ties5": lambda: tie_scenario(5),
    "merges3": lambda: merge_scenario(3), "merges4": lambda: merge_scenario(4),
    "K1": lambda: random_scenario(1, 3, 11, 0), "K4": lambda: random_scenario(4, 9, 12, 1),
    "K16": lambda: random_scenario(16, 5, 11, 0), "nan": lambda: random_scenario(3, 4, 14, 0, nan_at=(2, 3)),
}


def check_scenario(name, sc, ref, g):
    """What a scenario is there to show, asserted on the restatement (CPU and GPU tests alike)."""
    best = [beam[0] for beam in ref.beams if beam]
    if name.startswith("flip"):
        assert [e[0] for e in best] == [(2, 4, 6), (2, 4, 6)]
        plain = ds.BeamRestatement(ref.fn, sc.B, sc.K, sc.frames, sc.maxT, sc.blank)
        for _ in range(sc.steps):
            plain.step()
        assert [beam[0][0] for beam in plain.beams] == [(1, 3, 5), (1, 3, 5)]  # the unfused best
    if name == "depth":
        q = g.walk(DEPTH_PATH)[0]
        assert g.depth[q] == 8
        seen = {}
        for y, _, _ in ref.beams[0]:
            if y[:-1] == DEPTH_PATH:
                _, _, hop, arc = array_delta(g, q, y[-1], sc.blank, hops=True)
                seen[y[-1]] = (hop, arc)
        assert seen == {1: (0, True), 9: (1, True), 10: (2, True), 11: (4, True), 3: (8, True), 8: (8, False)}, seen
    if name.startswith("posbow"):
        q1 = g.walk((1,))[0]
        assert float(g.backoff_score[q1]) == 1.5 and float(g.delta(q1, 3)[1]) == 0.5 and best[0][0] == (1, 3, 5)
    if name.startswith("merges"):
        assert ref.ev.merges >= 4  # (identical sequences with identical states: asserted by the restatement at every merge)
