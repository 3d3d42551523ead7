"""Batched greedy TDT decoding: a float64 restatement of the step rule of include/rnnt_tdt_greedy.h, scripted scenarios and the
driver that plays the caller (a helper module, not a conftest).

TDTRestatement is written from the header text alone and shares nothing with tdt.py.  It works on the logits a
`logits_fn(b, t, tokens)` returns: [V + D] numbers, V token logits then D duration logits -- on the GPU the f32 logits of
compute_rnnt_joint_logits for that hypothesis alone with alphabet_size = V + D (both argmaxes are then exact, by the bitwise
guarantee of the header, so no case is skipped or excused there), on the CPU the script's own float64 table.

A Case holds what the caller of the C ABI holds: W2 [J, V + D], b2, enc_proj [B, T, J] and pred_row(b, t, tokens) -> the pred_proj
row of a hypothesis.  ScriptedCase makes one of tests/decode_scripts.ScriptedJoint with V + D columns: W2 = c I, enc_proj = 0, so
the logits are c tanh(pred_proj) and a scenario scripts them, exact ties included.

Comparison rules (run_tdt): ids, frames, lengths, emitted and all_done exactly, at every step, nothing skipped; scores and
per-token log-probabilities within the bar the calling test passes.  Where ties are not declared, the two best entries of each head
must be more than `min_gap` apart, asserted on the restatement alone.
"""
import math
from dataclasses import dataclass, field

import numpy as np

from tests.decode_scripts import ScriptedJoint

# every duration set of tests/test_tdt_loss.py: with and without 0, D = 1, D = 8 with a gap
DURATION_SETS = [[0, 1, 2], [1, 2], [0, 1, 2, 3, 4], [0, 1], [0, 2], [1], [0, 1, 2, 3], [0, 1, 2, 3, 4, 5, 6, 8]]


def _logsumexp(x):
    m = x.max()
    if not math.isfinite(m):
        return float("nan") if (m != m or m > 0) else -math.inf
    return float(m + math.log(np.exp(x - m).sum()))


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
@dataclass
class Events:
    steps: int = 0
    token_ties: int = 0
    duration_ties: int = 0
    min_gap: float = math.inf
    max_lse: float = 0.0
    paused_steps: int = 0
    capped: int = 0           # d = 0 emissions turned into d = 1 by max_per_frame
    blank_d0: int = 0         # blanks with d = 0 (moved on by one frame)
    zero_chains: int = 0      # emissions with d = 0 that stayed on their frame
    jumps_past_end: int = 0   # last jumps that landed beyond T_b
    jumps_from_last: int = 0  # ... taken from t = T_b - 1 with d > 1
    no_finite: int = 0        # heads without a finite logit
    blanks: int = 0
    durations_used: set = field(default_factory=set)


class TDTRestatement:
    """The step rule of include/rnnt_tdt_greedy.h in float64, one hypothesis at a time."""

    def __init__(self, logits_fn, B, V, durations, frame_lengths, max_symbols, max_per_frame, maxT, blank, ties_allowed=False,
                 min_gap=1e-6):
        assert max_per_frame >= 1 and 0 <= blank < V
        self.fn, self.B, self.V, self.dur, self.blank = logits_fn, B, V, list(durations), blank
        self.cap, self.ties_allowed, self.min_gap = int(max_per_frame), ties_allowed, min_gap
        self.Tb = [min(max(int(f), 0), maxT) for f in frame_lengths]
        self.maxsym = [None if max_symbols is None else max(int(max_symbols[b]), 0) for b in range(B)]
        self.t, self.nf, self.steps = [0] * B, [0] * B, [0] * B
        self.y, self.frames, self.logp = [()] * B, [()] * B, [()] * B
        self.score = [0.0] * B
        self.done = [self.Tb[b] == 0 or self.maxsym[b] == 0 for b in range(B)]
        self.ev = Events()

    def runs(self, b, max_hyp_len):
        lim = max_hyp_len if self.maxsym[b] is None else min(self.maxsym[b], max_hyp_len)
        return not self.done[b] and len(self.y[b]) < lim

    def _argmax(self, head, what):
        """-> (index or None when the head has no finite logit, the logit there)."""
        if not np.isfinite(head).any():
            self.ev.no_finite += 1
            return None, float("nan")
        k = int(np.argmax(head))  # (lowest index on ties)
        if head.shape[0] > 1:
            gap = float(head[k] - np.delete(head, k).max())
            if gap == 0.0:
                assert self.ties_allowed, f"scenario precondition: unintended tie in the {what} head"
                if what == "token":
                    self.ev.token_ties += 1
                else:
                    self.ev.duration_ties += 1
            else:
                self.ev.min_gap = min(self.ev.min_gap, gap)
                assert gap > self.min_gap, f"scenario precondition: {what} argmax {gap:.3e} ahead"
        return k, float(head[k])

    def step(self, max_hyp_len):
        """-> (emitted, all_done) as the library must write them; everything else is the object's state."""
        emitted = [-1] * self.B
        V, ev = self.V, self.ev
        for b in range(self.B):
            if not self.runs(b, max_hyp_len):
                continue
            lg = np.asarray(self.fn(b, self.t[b], self.y[b]), np.float64)
            assert lg.shape == (V + len(self.dur),)
            k, lk = self._argmax(lg[:V], "token")
            i, li = self._argmax(lg[V:], "duration")
            lse_t, lse_d = _logsumexp(lg[:V]), _logsumexp(lg[V:])
            for x in (lse_t, lse_d):
                if math.isfinite(x):
                    ev.max_lse = max(ev.max_lse, abs(x))
            lp = (lk - lse_t) + (li - lse_d)
            self.score[b] += lp
            self.steps[b] += 1
            d = 1 if i is None else self.dur[i]
            if i is not None:
                ev.durations_used.add(d)
            t0 = self.t[b]
            if k is not None and k != self.blank:
                self.y[b] += (k,)
                self.frames[b] += (t0,)
                self.logp[b] += (lp,)
                self.nf[b] += 1
                emitted[b] = k
                if d == 0 and self.nf[b] >= self.cap:
                    d = 1
                    ev.capped += 1
                elif d == 0:
                    ev.zero_chains += 1
            else:
                ev.blanks += 1
                if d == 0:
                    d = 1
                    ev.blank_d0 += 1
            if d > 0:
                self.nf[b] = 0
            self.t[b] += d
            if self.t[b] > self.Tb[b]:
                ev.jumps_past_end += 1
                ev.jumps_from_last += t0 == self.Tb[b] - 1
            if self.t[b] >= self.Tb[b] or (self.maxsym[b] is not None and len(self.y[b]) >= self.maxsym[b]):
                self.done[b] = True
        running = [b for b in range(self.B) if not self.done[b] and len(self.y[b]) < max_hyp_len]
        paused = [b for b in range(self.B) if not self.done[b] and len(self.y[b]) >= max_hyp_len]
        all_done = 0 if running else (2 if paused else 1)
        ev.steps += 1
        ev.paused_steps += all_done == 2
        return emitted, all_done


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    dtype: int          # joint_dtype
    J: int
    V: int
    durations: list
    B: int
    maxT: int
    frames: list
    max_symbols: object
    max_per_frame: int
    blank: int
    hyp_lens: list
    W2: np.ndarray       # [J, V + D] float32
    b2: np.ndarray       # [V + D] float32
    enc_proj: np.ndarray  # [B, maxT, J] float32
    pred_row: object     # (b, t, tokens) -> [J] float32
    script: object = None  # (b, t, tokens) -> [V + D] float64: the CPU logits of a scripted case
    ties_allowed: bool = False
    final_all_done: int = 1

    @property
    def D(self):
        return len(self.durations)

    @property
    def R(self):
        return self.V + len(self.durations)


def scripted_case(name, dtype, V, durations, B, maxT, frames, max_symbols, max_per_frame, blank, script, hyp_lens, ties_allowed=False,
                  final_all_done=1, c=16.0):
    """W2 = c I over V + D columns (J = 64 for joint_dtype 0: V + D <= 32; J = 128 for joint_dtype 1), enc_proj = 0."""
    R = V + len(durations)
    sj = ScriptedJoint(64 if dtype == 0 else 128, R, c, dtype)
    W2, b2 = sj.weights()
    snapped = lambda b, t, y: sj.snap(script(b, t, y))  # noqa: E731  (what survives the binary16 rounding of h)
    return Case(name, dtype, sj.J, V, list(durations), B, maxT, list(frames), max_symbols, max_per_frame, blank, list(hyp_lens), W2, b2,
                sj.enc_proj(B, maxT), lambda b, t, y: sj.pred_rows(script(b, t, y))[0], snapped, ties_allowed, final_all_done)


def _h(*key):
    h = 1469598103
    for k in key:
        h = (h * 1000003 + int(k) * 7919 + 12345) % 2147483647
    return h


def head_script(seed, V, durations, blank, blank_rate=3, dur_of=None, tok_of=None):
    """The wanted token at logit 0 and the wanted duration index at logit 0, the others 0.5 apart below (from the 12th on: -6).
    tok_of(b, t, y) / dur_of(b, t, y) -> a token / a duration INDEX, or None for the pseudo-random choice."""
    D = len(durations)

    def script(b, t, y):
        h = _h(seed, b, t, len(y))
        k = tok_of(b, t, y) if tok_of else None
        if k is None:
            if h % blank_rate:
                k = (h // 7) % (V - 1)
                k += k >= blank
            else:
                k = blank
        i = dur_of(b, t, y) if dur_of else None
        if i is None:
            i = (h // 131) % D
        L = np.empty(V + D)
        L[:V] = -0.5 * np.minimum((np.arange(V) - k) % V, 12)
        L[V:] = -0.5 * np.minimum((np.arange(D) - i) % D, 12)
        return L

    return script


def tie_script(V, durations, blank, toks):
    """Exact ties in both heads by frame: tokens (s0, s1), (blank, s1), (s0, blank), alone; durations (0, 1), (1, last), alone.
    s0 < blank < s1.  A third entry sits 0.75 below."""
    s0, s1 = toks
    D = len(durations)
    assert s0 < blank < s1 < V and D >= 3
    tpairs = [(s0, s1), (blank, s1), (s0, blank), (s1, s1)]
    dpairs = [(0, 1), (1, D - 1), (D - 1, D - 1)]

    def script(b, t, y):
        L = np.full(V + D, -5.0)
        x, z = tpairs[(t + b + len(y)) % 4]
        L[x] = L[z] = 0.0
        L[[v for v in range(V) if v not in (x, z)][0]] = -0.75
        p, q = dpairs[(t + 2 * b + len(y)) % 3]
        L[V + p] = L[V + q] = 0.0
        L[V + [j for j in range(D) if j not in (p, q)][0]] = -0.75
        return L

    return script


def duration_set_case(durations, dtype=0, V=9, blank=0):
    """A ragged batch over one duration set: empty utterances, lengths above maxT, budgets of 0 and 1, blank first / middle / last
    by the caller's choice of `blank`."""
    B, T = 7, 24
    frames = [T, 0, 1, T + 3, 5, 2, T]
    max_symbols = [1000, 5, 1000, 0, 1, 1000, 3]
    return scripted_case(f"durations-{durations}-blank{blank}-dt{dtype}", dtype, V, durations, B, T, frames, max_symbols, 3, blank,
                         head_script(len(durations) * 17 + durations[-1], V, durations, blank), [128])


def zero_chain_case(dtype=0, cap=3):
    """Every decision a token with d = 0: only the cap moves the frame on (durations [0, 1, 2], index 0 forced)."""
    V, dur = 7, [0, 1, 2]
    tok = lambda b, t, y: 1 + (len(y) + b) % (V - 1)  # noqa: E731  (never the blank 0)
    return scripted_case(f"zero-chain-cap{cap}-dt{dtype}", dtype, V, dur, 3, 4, [4, 2, 6], None, cap, 0,
                         head_script(5, V, dur, 0, dur_of=lambda b, t, y: 0, tok_of=tok), [64])


def blank_zero_case(dtype=0):
    """Every decision the blank with d = 0: one frame per step."""
    V, dur = 6, [0, 1, 3]
    return scripted_case(f"blank-d0-dt{dtype}", dtype, V, dur, 2, 5, [5, 3], None, 2, 2,
                         head_script(6, V, dur, 2, dur_of=lambda b, t, y: 0, tok_of=lambda b, t, y: 2), [8])


def jump_past_end_case(dtype=0):
    """d = 1 up to t = T_b - 1, then the largest duration: the last jump passes T_b.  Row 2 emits a token on that last frame."""
    V, dur = 6, [0, 1, 2, 4]
    frames = [5, 1, 3, 2]
    last = lambda b, t: t == min(frames[b], 5) - 1  # noqa: E731
    dur_of = lambda b, t, y: 3 if last(b, t) else 1  # noqa: E731
    tok_of = lambda b, t, y: (3 if b == 2 and last(b, t) else (0 if last(b, t) else None))  # noqa: E731
    return scripted_case(f"jump-past-end-dt{dtype}", dtype, V, dur, 4, 5, frames, None, 2, 0,
                         head_script(7, V, dur, 0, dur_of=dur_of, tok_of=tok_of), [16])


def pause_case(hyp_lens, dtype=1):
    """Tokens all the time on long utterances: the hyps buffer fills, the decode pauses (all_done = 2) and resumes when grown."""
    V, dur = 40, [0, 1, 2]
    B, T = 6, 7
    return scripted_case("pause", dtype, V, dur, B, T, [T, 3, T + 1, 0, T, 5], None, 2, 9,
                         head_script(77, V, dur, 9, blank_rate=5), list(hyp_lens))


def tie_case(dtype):
    V, dur, blank = (100, [0, 1, 2, 3], 40) if dtype else (20, [0, 1, 2, 3], 9)
    toks = (3, 70) if dtype else (2, 13)
    return scripted_case(f"ties-dt{dtype}", dtype, V, dur, 5, 8, [8, 8, 0, 10, 5], None, 2, blank, tie_script(V, dur, blank, toks), [40],
                         ties_allowed=True)


def nan_row_case(dtype=0):
    """A row of NaN at (utterance 1, frame 2): neither head has a finite logit -- blank, d = 1, a NaN score for that utterance."""
    V, dur = 8, [0, 1, 2]
    base = head_script(9, V, dur, 0)

    def script(b, t, y):
        return np.full(V + len(dur), np.nan) if (b, t) == (1, 2) else base(b, t, y)

    return scripted_case(f"nan-row-dt{dtype}", dtype, V, dur, 3, 6, [6, 6, 4], None, 2, 0, script, [32])


def scripted_scenarios(dtype):
    """The CPU scenarios, for one joint_dtype (every duration set with the blank first; blank middle / last on two of them)."""
    out = [duration_set_case(d, dtype) for d in DURATION_SETS]
    out += [duration_set_case([0, 1, 2, 3, 4], dtype, blank=4), duration_set_case([1, 2], dtype, blank=8)]
    out += [zero_chain_case(dtype, 3), zero_chain_case(dtype, 1), blank_zero_case(dtype), jump_past_end_case(dtype), pause_case([5, 10, 40], dtype),
            tie_case(dtype), nan_row_case(dtype)]
    return out


# ---------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------
def run_tdt(engine, case, logits_fn, score_bar, logp_bar, check=True, min_gap=1e-6, max_steps=100000):
    """Play the caller of compute_rnnt_tdt_greedy_*: `engine` has begin(max_hyp_len), step(rows [B, J]) -> (emitted, all_done,
    lengths, scores, hyps, frames or None, logp or None) and grow(max_hyp_len), all numpy.  case.hyp_lens: the buffer sizes to go
    through, each used until all_done != 0 (2: on to the next).  Rows that are done or paused get NaN pred_proj: they read nothing.
    score_bar(n, max_lse, s) / logp_bar(max_lse, lp): the allowed errors.  -> (trace, restatement, worst score error, its bar,
    worst log-probability error, its bar)."""
    ref = TDTRestatement(logits_fn, case.B, case.V, case.durations, case.frames, case.max_symbols, case.max_per_frame, case.maxT,
                         case.blank, case.ties_allowed, min_gap)
    trace = []
    hyp_lens = list(case.hyp_lens)
    N = hyp_lens.pop(0)
    engine.begin(N)
    worst, worst_bar, lworst, lworst_bar = 0.0, 0.0, 0.0, 0.0
    B = case.B
    for _ in range(max_steps):
        rows = np.full((B, case.J), np.nan, np.float32)
        for b in range(B):
            if ref.runs(b, N):
                rows[b] = case.pred_row(b, ref.t[b], ref.y[b])
        out = engine.step(rows)
        emitted, all_done, lengths, scores, hyps, frames, logp = out
        trace.append(tuple(np.array(x).copy() for x in out if x is not None))
        want_e, want_d = ref.step(N)
        if check:
            at = len(trace)
            assert emitted.tolist() == want_e, (at, "emitted", emitted.tolist(), want_e)
            assert int(all_done) == want_d, (at, "all_done", int(all_done), want_d)
            assert lengths.tolist() == [len(y) for y in ref.y], (at, "lengths")
            for b in range(B):
                n = len(ref.y[b])
                assert hyps[b, :n].tolist() == list(ref.y[b]), (at, b, "ids")
                assert not hyps[b, n:].any(), (at, b, "nothing else is written to hyps")
                s = ref.score[b]
                if s != s:
                    assert scores[b] != scores[b], (at, b, "the score must be NaN", float(scores[b]))
                else:
                    err, bar = abs(float(scores[b]) - s), score_bar(ref.steps[b], ref.ev.max_lse, s)
                    assert err <= bar, (at, b, "score", float(scores[b]), s, err, bar)
                    if err >= worst:
                        worst, worst_bar = err, bar
                if frames is not None:
                    assert frames[b, :n].tolist() == list(ref.frames[b]), (at, b, "frames")
                    assert (frames[b, n:] == -1).all() and not logp[b, n:].any(), (at, b, "nothing else is written to the times")
                    for j, lp in enumerate(ref.logp[b]):
                        if lp != lp:
                            assert logp[b, j] != logp[b, j], (at, b, j, "the log-probability must be NaN")
                            continue
                        err, bar = abs(float(logp[b, j]) - lp), logp_bar(ref.ev.max_lse, lp)
                        assert err <= bar, (at, b, j, "logp", float(logp[b, j]), lp, err, bar)
                        if err >= lworst:
                            lworst, lworst_bar = err, bar
        if want_d == 0:
            continue
        if want_d == 2 and hyp_lens:
            N = hyp_lens.pop(0)
            engine.grow(N)
            continue
        break
    else:
        raise AssertionError("the scripted decode did not end")
    if check:
        assert want_d == case.final_all_done, (want_d, case.final_all_done)
    return trace, ref, worst, worst_bar, lworst, lworst_bar


def traces_equal(a, b) -> bool:
    """Bitwise equality of two traces (scores compared as bits: NaN payloads included)."""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if len(x) != len(y):
            return False
        for p, q in zip(x, y):
            p, q = np.asarray(p), np.asarray(q)
            if p.shape != q.shape or p.dtype != q.dtype or p.tobytes() != q.tobytes():
                return False
    return True


def host_loop_decode(tdt_greedy_decode, logits_fn, case, b):
    """tdt.tdt_greedy_decode for utterance b of a case without a symbol budget -> (tokens, frames)."""
    T = min(max(int(case.frames[b]), 0), case.maxT)
    return tdt_greedy_decode(lambda t, y: logits_fn(b, t, tuple(y)), T, case.durations, case.blank, case.max_per_frame)


def describe(case, ev, worst, bar, lworst, lbar):
    gap = "-" if ev.min_gap == math.inf else f"{ev.min_gap:.3g}"
    return (f"[{case.name}] steps={ev.steps} token-ties={ev.token_ties} duration-ties={ev.duration_ties} capped={ev.capped} "
            f"d0-chains={ev.zero_chains} blank-d0={ev.blank_d0} jumps-past-end={ev.jumps_past_end} (from T-1: {ev.jumps_from_last}) "
            f"no-finite-heads={ev.no_finite} paused-steps={ev.paused_steps} durations-used={sorted(ev.durations_used)} min-gap={gap} "
            f"score-error={worst:.3e} bar={bar:.3e} logp-error={lworst:.3e} bar={lbar:.3e}")
