"""Streaming TDT beam search over slots (include/rnnt_tdt_beam_stream.h): scenarios and the driver that plays the caller (a helper
module, not a conftest).  The reference is tests/tdt_beam_cases.TDTBeamRestatement, imported as it is, on each stream's WHOLE
utterance (one utterance, one chunk): chunking, slots, carries and restarts exist on the decoder's side alone.  The one rule the
offline restatement cannot hold, the capacity rule (a hypothesis with N tokens offers its blank alone), is restated in NRule.

A Scenario holds streams over one tests/tdt_decode_cases.Case (W2 = c I over V + D columns; utterance `key` of the case is what a
stream decodes).  The decoder's W1 and b1 are ZERO, so enc_proj is exactly 0 on every route whatever the encoder frames hold, and the
logits are c tanh(pred_proj): those of the case.  A stream lives in a slot from its `start` feed on and brings chunks[k] frames at
feed start + k, the final flag on its last chunk; `after` are frames fed to the slot once it is finished (they must change nothing).
A later stream in the same slot restarts it.

run_streams feeds them and steps max(frames) times after every feed, and holds the decoder against the restatements at EVERY step:
parents and emitted (frozen slots: own row, -1), ids, lengths, cursors, frames, durations and both stable lengths exactly; scores
by the callable the test passes.  Rows that are not active get NaN pred_proj: they must read nothing.  With `tops` the engine's
token diagnostics are held against the plain top-`beam` of the row.

An engine has begin(), feed(enc [S, Te, H] or None, frames, reset, final), step(rows [S K, J]) -> (parents, emitted) (after which
engine.tops is None or the step's topk_symbols [S K, K], -7 where not written) and results() -> (hyps [S, K, N], lengths, scores,
stable, cursors, frames, durations, timed_stable); all numpy."""
import math
from dataclasses import dataclass, field

import numpy as np

from tests import tdt_beam_cases as bc
from tests import tdt_decode_cases as tc

H = 8  # the encoder width of every scenario (W1 = 0: the frames' values never matter)


class NRule(bc.TDTBeamRestatement):
    """The restatement with the capacity rule: an active hypothesis that holds N tokens offers only (blank, j) for every j, scored
    against the logsumexp of its WHOLE token row.  Everything else is the parent's rule, restated without its bookkeeping
    (tests/test_tdt_beam_stream.py holds the two against each other where the rule cannot fire)."""

    def __init__(self, *args, N, **kw):
        super().__init__(*args, **kw)
        self.N, self.full_rows, self.mixed_frames, self.blank_outside = N, 0, 0, 0

    def step(self):
        K, V, t, D = self.K, self.V, self.t, len(self.dur)
        parents, emitted = list(range(self.B * K)), [-1] * (self.B * K)
        for b in range(self.B):
            if t >= self.Tb[b]:
                continue
            beam, cands, kinds = self.beams[b], [], set()
            for i, (y, c, s, fr, du) in enumerate(beam):
                if c != t:
                    cands.append((s, i, 0, -1, -1))
                    continue
                lg = np.asarray(self.fn(b, t, y), np.float64)
                lt, ld = tc._logsumexp(lg[:V]), tc._logsumexp(lg[V:])
                full = len(y) >= self.N
                kinds.add(full)
                self.full_rows += full
                self.blank_outside += full and sum(1 for v in range(V) if (-lg[v], v) < (-lg[self.blank], self.blank)) >= K
                for v in ([self.blank] if full else range(V)):
                    for j in range(D):
                        sc = s + ((lg[v] - lt) + (lg[V + j] - ld))
                        if sc == sc and sc > -math.inf:
                            cands.append((float(sc), i, 1, v, j))
            self.mixed_frames += kinds == {False, True}
            cands.sort(key=lambda x: (-x[0], x[1], x[2], x[3], x[4]))
            for p, q in zip(cands[:K], cands[1:K + 1]):
                self._gap(p[0], q[0], t + 1, f"utterance {b} frame {t}")
            if not cands:
                self.beams[b] = [(y, t + 1, s, fr, du) for y, c, s, fr, du in beam]
                continue
            new = []
            for sc, i, kind, v, j in cands[:K]:
                y, c, _, fr, du = beam[i]
                em = -1
                if kind == 1:
                    d = self.dur[j] or 1
                    c = t + d
                    if v != self.blank:
                        y, fr, du, em = y + (v,), fr + (t,), du + (d,), v
                hit = next((e for e in new if e[0] == y and e[1] == c), None)
                if hit is None:
                    new.append([y, c, sc, fr, du, i, em])
                else:
                    hit[2] = bc._logaddexp(hit[2], sc)
            new.sort(key=lambda e: -e[2])  # (stable)
            self.beams[b] = [tuple(e[:5]) for e in new]
            for k, e in enumerate(new):
                parents[b * K + k], emitted[b * K + k] = b * K + e[5], e[6]
        self.t += 1
        return parents, emitted


@dataclass
class Stream:
    slot: int
    key: int  # the utterance of the case it decodes
    T: int
    chunks: list
    start: int = 0
    after: list = field(default_factory=list)


@dataclass
class Scenario:
    name: str
    case: object  # tests/tdt_decode_cases.Case; case.B utterances of case.maxT frames
    K: int
    S: int
    Tc: int
    N: int
    streams: list
    n_rule: bool = False  # the reference is NRule (N below the frames of a stream)


@dataclass
class Outcome:
    refs: list
    results: list  # per stream: results() rows of its slot as last reported while the stream owned it
    feeds: int = 0
    steps: int = 0
    frozen_steps: int = 0  # (slot, step) pairs where a slot with a stream had no frame left
    tops_checked: int = 0


def make_ref(sc, st, logits_fn):
    case = sc.case
    fn = lambda b, t, y: logits_fn(st.key, t, y)  # noqa: E731
    args = (fn, 1, sc.K, case.V, case.durations, [st.T], st.T, case.blank, case.ties_allowed)
    return NRule(*args, N=sc.N) if sc.n_rule else bc.TDTBeamRestatement(*args)


def _prefix(beam, *fields):
    n = min((len(h[0]) for h in beam), default=0)
    for p in range(n):
        if any(h[f][p] != beam[0][f][p] for h in beam for f in fields):
            return p
    return n


def run_streams(engine, sc, logits_fn, score_ok, enc_seed=0):
    """-> Outcome.  score_ok(got, want, steps, ref) -> bool."""
    case, K, S, N = sc.case, sc.K, sc.S, sc.N
    rng = np.random.default_rng(enc_seed)
    out = Outcome([make_ref(sc, st, logits_fn) for st in sc.streams], [None] * len(sc.streams))
    owner = [None] * S  # the stream in a slot
    seqs = [()] * (S * K)
    engine.begin()
    n_feeds = max(st.start + len(st.chunks) + len(st.after) for st in sc.streams)

    def compare(what):
        res = engine.results()
        hyps, lengths, scores, stable, cursors, frames, durs, tstable = res
        for s in range(S):
            at = (what, "slot", s)
            beam = [] if owner[s] is None else out.refs[owner[s]].beams[0]
            for k in range(K):
                if k >= len(beam):
                    assert lengths[s, k] == 0 and scores[s, k] == -math.inf and not hyps[s, k].any() and cursors[s, k] == -1, (at, k, "empty")
                    assert frames is None or ((frames[s, k] == -1).all() and (durs[s, k] == -1).all()), (at, k, "empty times")
                    continue
                y, c, sco, fr, du = beam[k]
                L = len(y)
                assert lengths[s, k] == L and hyps[s, k, :L].tolist() == list(y) and not hyps[s, k, L:].any(), (at, k, "ids")
                assert cursors[s, k] == c, (at, k, "cursor", int(cursors[s, k]), c)
                if frames is not None:
                    assert frames[s, k, :L].tolist() == list(fr) and (frames[s, k, L:] == -1).all(), (at, k, "frames")
                    assert durs[s, k, :L].tolist() == list(du) and (durs[s, k, L:] == -1).all(), (at, k, "durations")
                assert seqs[s * K + k] == y, (at, k, "the caller's sequence")
                assert score_ok(float(scores[s, k]), sco, out.refs[owner[s]].t, out.refs[owner[s]]), (at, k, "score", float(scores[s, k]), sco)
            assert stable[s] == _prefix(beam, 0), (at, "stable", int(stable[s]))
            if tstable is not None:
                assert tstable[s] == _prefix(beam, 0, 3, 4) <= stable[s], (at, "timed stable", int(tstable[s]))
            if owner[s] is not None:
                out.results[owner[s]] = tuple(None if x is None else np.array(x[s]).copy() for x in res)

    for f in range(n_feeds):
        fr, rs, fi = [0] * S, [0] * S, [0] * S
        left = [0] * S  # the frames of this feed a slot's stream will decode
        for n, st in enumerate(sc.streams):
            k = f - st.start
            if k == 0:
                owner[st.slot], rs[st.slot] = n, 1
                seqs[st.slot * K: st.slot * K + K] = [()] * K
            if 0 <= k < len(st.chunks) and owner[st.slot] == n:
                fr[st.slot], fi[st.slot] = st.chunks[k], int(k + 1 == len(st.chunks))
                left[st.slot] = st.chunks[k]
            elif len(st.chunks) <= k < len(st.chunks) + len(st.after) and owner[st.slot] == n:
                fr[st.slot] = st.after[k - len(st.chunks)]  # (a finished slot: the frames are ignored)
        Te = max(fr)
        assert Te <= sc.Tc
        enc = rng.standard_normal((S, Te, H)).astype(np.float32) if Te else None
        engine.feed(enc, fr, rs, fi)
        out.feeds += 1
        compare(("feed", f))
        for step in range(Te):
            rows = np.full((S * K, case.J), np.nan, np.float32)
            live = [s for s in range(S) if left[s] > 0]
            for s in live:
                ref, st = out.refs[owner[s]], sc.streams[owner[s]]
                for k in range(K):
                    if ref.active(0, k):
                        rows[s * K + k] = case.pred_row(st.key, ref.t, seqs[s * K + k])
            parents, emitted = engine.step(rows)
            out.steps += 1
            want_p, want_e = list(range(S * K)), [-1] * (S * K)
            for s in range(S):
                if s not in live:
                    out.frozen_steps += owner[s] is not None
                    continue
                ref, st = out.refs[owner[s]], sc.streams[owner[s]]
                tops = getattr(engine, "tops", None)
                if tops is not None:  # the token diagnostics: the plain top-K of every active row, full or not
                    for k in range(K):
                        if ref.active(0, k):
                            lg = np.asarray(logits_fn(st.key, ref.t, ref.beams[0][k][0]))[: case.V]
                            order = sorted((v for v in range(case.V) if lg[v] == lg[v] and lg[v] > -math.inf), key=lambda v: (-float(lg[v]), v))[:K]
                            got = tops[s * K + k]
                            assert got[: len(order)].tolist() == order and (got[len(order):] == -1).all(), (f, step, s, k, got, order)
                            out.tops_checked += 1
                p, e = ref.step()
                want_p[s * K: s * K + K] = [s * K + x for x in p]
                want_e[s * K: s * K + K] = e
                left[s] -= 1
            assert parents.tolist() == want_p, (f, step, "parents", parents.tolist(), want_p)
            assert emitted.tolist() == want_e, (f, step, "emitted", emitted.tolist(), want_e)
            seqs = [seqs[p] + ((e,) if e >= 0 else ()) for p, e in zip(parents.tolist(), emitted.tolist())]
            compare(("feed", f, "step", step))
    for n, st in enumerate(sc.streams):
        if sum(st.chunks) == st.T and owner[st.slot] == n:
            assert out.refs[n].t == st.T, (n, "the stream was not decoded to its end")
    return out


def same_bits(a, b) -> bool:
    """Two streams' results, bit for bit (scores as bits)."""
    return all((x is None and y is None) or (x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------
# scenarios
# ---------------------------------------------------------------------------------------------
def _case(name, dtype, V, durations, keys, T, blank, script, ties_allowed=False, J=None):
    if J is None:
        return tc.scripted_case(name, dtype, V, durations, keys, T, [T] * keys, None, 1, blank, script, [T], ties_allowed=ties_allowed)
    from tests.decode_scripts import ScriptedJoint  # (a joint wider than scripted_case's: more than one slice of columns)

    sj = ScriptedJoint(J, V + len(durations), 16.0, dtype)
    W2, b2 = sj.weights()
    return tc.Case(name, dtype, J, V, list(durations), keys, T, [T] * keys, None, 1, blank, [T], W2, b2, sj.enc_proj(keys, T),
                   lambda b, t, y: sj.pred_rows(script(b, t, y))[0], lambda b, t, y: sj.snap(script(b, t, y)), ties_allowed)


D5, D8 = [0, 1, 2, 3, 4], [0, 1, 2, 8]
T13 = 13
CHUNKINGS = {"one": [13], "ones": [1] * 13, "zeros-between": [2, 0, 3, 0, 0, 1, 7], "cuts": [3, 1, 4, 5], "empty-final": [6, 7, 0]}
SEEDS = {(0, 4): 100, (1, 4): 100, (0, 1): 100, (0, 16): 100, (1, 16): 100}  # (joint_dtype, K) -> random_script's seed; see _seed


def _seed(dtype, K):
    return SEEDS.get((dtype, K), 100)


def chunking_scenario(name, K=4, dtype=0, slot=0, S=1, timed_N=T13):
    """One stream of 13 frames over durations [0, 1, 2, 3, 4] through CHUNKINGS[name]."""
    case = _case(f"chunks-{name}-K{K}-dt{dtype}", dtype, 9, D5, 1, T13, 0, bc.random_script(_seed(dtype, K), 9, 5, 0))
    return Scenario(case.name, case, K, S, T13, timed_N, [Stream(slot, 0, T13, CHUNKINGS[name])])


def long_carry_scenario(chunk, K=4, dtype=0):
    """Durations [0, 1, 2, 8] with the jump of 8 far ahead and chunks of `chunk` frames: a carry outlives several feeds, the frames
    between are idle with a full beam, and the last jump passes the stream's end."""
    T = 14
    case = _case(f"long-carry-{chunk}-K{K}-dt{dtype}", dtype, 20, D8, 1, T, 2, bc.long_jump_script(20, 4, 2, 3))
    chunks = [T] if chunk >= T else [chunk] * (T // chunk) + ([T % chunk] if T % chunk else [])
    return Scenario(case.name, case, K, 1, T, T, [Stream(0, 0, T, chunks)])


def boundary_merge_scenario(chunk, K=4, dtype=0):
    """bc.wait_merge_script over durations [1, 2, 4] in chunks of `chunk` frames: (y, t + 1) and (y, t + 2) are kept apart -- across
    a boundary when chunk = 1 --, and the expansion that lands on the waiting hypothesis's cursor after the next feed merges with
    its stay."""
    T = 9
    case = _case(f"boundary-merge-{chunk}-K{K}-dt{dtype}", dtype, 7, [1, 2, 4], 1, T, 0, bc.wait_merge_script(7, 3, 0, 0, 1))
    chunks = [T] if chunk >= T else [chunk] * (T // chunk) + ([T % chunk] if T % chunk else [])
    return Scenario(case.name, case, K, 1, T, T, [Stream(0, 0, T, chunks)])


def slots_scenario(slot, S=4, K=4, dtype=0):
    """The stream of chunking_scenario (key 0, chunks 3 1 4 5) in `slot`, beside streams that are reset, finished and fed other
    lengths in the same feeds; one of them is abandoned by a restart, one is fed after it finished."""
    case = _case(f"slots-{slot}of{S}-K{K}-dt{dtype}", dtype, 9, D5, 3, T13, 0, bc.random_script(_seed(dtype, K), 9, 5, 0))
    others = [s for s in range(S) if s != slot]
    streams = [Stream(slot, 0, T13, CHUNKINGS["cuts"], start=1)]
    streams.append(Stream(others[0], 1, T13, [5, 0, 2, 6], start=0, after=[3]))
    streams.append(Stream(others[1], 2, T13, [1, 1, 2, 9], start=0))           # abandoned after 2 frames ...
    streams.append(Stream(others[1], 1, T13, [7, 6], start=2, after=[2]))      # ... by this restart
    if len(others) > 2:
        streams.append(Stream(others[2], 2, T13, [13], start=2))
    return Scenario(case.name, case, K, S, T13, T13, streams)


def final_scenario(K=4, dtype=0):
    """A final chunk that cuts a stream short (9 of 13 frames: carries beyond it are dropped), frames fed to the finished slot, and a
    reset that reuses it for the whole utterance."""
    case = _case(f"final-K{K}-dt{dtype}", dtype, 9, D5, 2, T13, 0, bc.random_script(_seed(dtype, K), 9, 5, 0))
    streams = [Stream(0, 0, 9, [4, 5], start=0, after=[3, 2]), Stream(0, 0, T13, [13], start=4), Stream(1, 1, T13, [2, 2, 2, 2, 5], start=0)]
    return Scenario(case.name, case, K, 2, T13, T13, streams)


def full_script(V, D, blank):
    """Tokens in a close fan that moves with the frame; the blank is the LOWEST token logit at even frames (outside every top-K
    below V) and close to the top at odd frames, so beams hold full hypotheses beside shorter ones."""
    def script(b, t, y):
        L = np.empty(V + D)
        L[:V] = -0.4 * ((np.arange(V) + 2 * t + b) % V) - 0.13 * bc._u(V, 21, b, t, len(y), y[-1] if y else V)
        L[blank] = -7.5 if t % 2 == 0 else -0.9
        L[V:] = -1.1 * ((np.arange(D) + t) % D) - 0.2 * bc._u(D, 22, b, t, len(y))
        return L

    return script


def n_rule_scenario(N, K=4, dtype=0, chunks=(2, 1, 3, 4)):
    T = 10
    case = _case(f"n-rule-N{N}-K{K}-dt{dtype}", dtype, 9, [0, 1, 2], 1, T, 0, full_script(9, 3, 0))
    return Scenario(case.name, case, K, 1, T, N, [Stream(0, 0, T, list(chunks))], n_rule=True)


def nan_scenario(K=4, dtype=0):
    """One duration (every hypothesis always active): frame 4 is a row of NaN logits for every hypothesis -- nothing is taken, the
    beam is carried over and every cursor moves one frame on; from frame 6 on the hypotheses of odd length are NaN."""
    T = 9
    nan = lambda b, t, y: t == 4 or (t >= 6 and len(y) % 2 == 1)  # noqa: E731
    case = _case(f"nan-K{K}-dt{dtype}", dtype, 7, [1], 1, T, 0, bc.random_script(bc.NAN_SEED, 7, 1, 0, nan=nan))
    return Scenario(case.name, case, K, 2, T, T, [Stream(1, 0, T, [3, 2, 4])])


def geometry_scenario(S, K, slot, V=9, durations=D5, dtype=0, J=None, T=10, chunks=(3, 1, 2, 4)):
    """One short stream in `slot` of S (rows S K: across a 32-row tile, beyond 256 rows) beside a second one in the last slot."""
    D = len(durations)
    case = _case(f"geometry-S{S}-K{K}-V{V}-D{D}-dt{dtype}", dtype, V, durations, 2, T, 0, bc.random_script(100, V, D, 0), J=J)
    streams = [Stream(slot, 0, T, list(chunks))]
    if S > 1:
        streams.append(Stream(S - 1 if slot != S - 1 else 0, 1, T, [T], start=1))
    return Scenario(case.name, case, K, S, T, T, streams)
