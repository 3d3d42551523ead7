"""Streaming beam search with several symbols per frame over slots (include/rnnt_beam_multi_stream.h): scenarios and the driver that
plays the caller (a helper module, not a conftest).  The reference is tests/multibeam_cases.MultiRestatement, imported as it is, on
each stream's WHOLE utterance (one utterance, one chunk) at max_hyp_len = N: chunking, slots, frame bases and restarts exist on the
decoder's side alone.  FrameTracker adds what the new header adds: a frame row per hypothesis (the frame, counted from the stream's
start, whose joint evaluation appended each token), the merge rule (an entry of the closed list that a closing is added into keeps
ITS OWN frame row) and both stable lengths.

A Scenario holds streams over one scripted joint (tests/decode_scripts.ScriptedJoint: W2 = c I; `script(key, t, y)` gives the logits
of the hypothesis y of utterance `key` at its frame t).  The decoder's W1 is ZERO and b1 = 0, so enc_proj is exactly b1 on every
route whatever the encoder frames hold.  A stream lives in a slot from its `start` feed on and brings chunks[k] frames at feed
start + k, the final flag on its last chunk; `after` are frames fed to the slot once it is finished (they must change nothing).  A
later stream in the same slot restarts it.

run_streams feeds them, steps max(frames) (E + 1) times after every feed, and holds the decoder against the restatements: parents and
emitted at EVERY step (frozen slots: own row, -1), and after every feed and every whole frame the ids, lengths, frames and both
stable lengths exactly and the scores by the callable the test passes.  Rows that are not live get NaN pred_proj: they must read
nothing.

An engine has begin(), feed(enc [S, Te, H] or None, frames, reset, final), step(rows [S 2K, J]) -> (parents, emitted) and results()
-> (hyps [S, K, N], lengths, scores, stable, frames or None, timed_stable or None); all numpy."""
import math
from dataclasses import dataclass, field

import numpy as np

from tests import decode_scripts as ds
from tests import multibeam_cases as mc

H = 8  # the encoder width of every scenario (W1 = 0: the frames' values never matter)


# ---------------------------------------------------------------------------------------------
# the reference: the restatement of one whole stream, with frames
# ---------------------------------------------------------------------------------------------
def prefix(beam_fields) -> int:
    """beam_fields: per hypothesis a tuple of equally long rows -> the leading positions on which all hypotheses agree in all."""
    if not beam_fields:
        return 0
    n = min(len(h[0]) for h in beam_fields)
    for p in range(n):
        if any(row[p] != first[p] for h in beam_fields for row, first in zip(h, beam_fields[0])):
            return p
    return n


class FrameTracker:
    """mc.MultiRestatement of ONE stream (B = 1) and, per row of its 2 K rows, the frame row of the hypothesis there.  The frame
    rows follow the header: an expansion appends the frame of the evaluation to its parent's row; a closing takes its hypothesis's
    row along; an entry of the closed list that a closing is ADDED INTO keeps its own row (asserted here, with the count of such
    merges whose two members differ in frames, and of those that reach list A at the frame turn)."""

    def __init__(self, logits_fn, key, K, E, N, T, blank, ties_allowed=False):
        self.ref = mc.MultiRestatement(lambda b, t, y: logits_fn(key, t, y), 1, K, E, N, [T], T, blank, ties_allowed)
        self.K, self.E, self.T = K, E, T
        self.rows = [()] * (2 * K)
        self.frame_merges, self.frame_merges_reported, self._merged = 0, 0, set()

    @property
    def frame(self):
        return self.ref.k // (self.E + 1)

    @property
    def done(self):
        return self.frame >= self.T

    def open(self):
        """List A: [(tokens, score, frames)]."""
        return [(y, s, self.rows[k]) for k, (y, s) in enumerate(self.ref.open[0])]

    def step(self):
        K, ref = self.K, self.ref
        t, rnd = divmod(ref.k, self.E + 1)
        A = [(y, self.rows[k]) for k, (y, _) in enumerate(ref.open[0])]
        Bl = {y: self.rows[K + j] for j, (y, _) in enumerate(ref.closed[0])}
        merges = ref.ev.closed_merges
        parents, emitted = ref.step()
        self.rows = [self.rows[p] + ((t,) if e >= 0 else ()) for p, e in zip(parents, emitted)]
        after = ref.open[0] if rnd == self.E else ref.closed[0]
        base = 0 if rnd == self.E else K
        if ref.ev.closed_merges > merges:  # a closing was added into an older entry: the entry's own row survives
            for y, fr in A:
                if y in Bl and Bl[y] != fr:
                    self.frame_merges += 1
                    self._merged.add(y)
                    for k, (y2, _) in enumerate(after):
                        if y2 == y:
                            assert self.rows[base + k] == Bl[y] != fr, "the entry must keep its own frame row"
        if rnd == self.E:
            self.frame_merges_reported += sum(1 for y, _ in ref.open[0] if y in self._merged)
            self._merged = set()
        for k, (y, _) in enumerate(ref.open[0]):
            assert len(self.rows[k]) == len(y)
        return parents, emitted

    def stable(self):
        return prefix([(y,) for y, _, _ in self.open()])

    def timed_stable(self):
        return prefix([(y, fr) for y, _, fr in self.open()])


@dataclass
class Stream:
    slot: int
    key: int  # the utterance of the script it decodes
    T: int
    chunks: list
    start: int = 0
    after: list = field(default_factory=list)


@dataclass
class Scenario:
    name: str
    dtype: int
    V: int
    K: int
    E: int
    S: int
    Tc: int
    N: int
    blank: int
    script: object
    streams: list
    ties_allowed: bool = False
    J: int = 0  # 0: 64 for joint_dtype 0, 128 for joint_dtype 1
    expect: dict = field(default_factory=dict)  # lower bounds on the summed MultiEvents counters and FrameTracker counts

    @property
    def joint(self):
        return ds.ScriptedJoint(self.J or (64 if self.dtype == 0 else 128), self.V, 16.0, self.dtype)


@dataclass
class Outcome:
    refs: list
    results: list  # per stream: results() rows of its slot as last reported while the stream owned it
    feeds: int = 0
    steps: int = 0
    frozen_steps: int = 0  # (slot, step) pairs where a slot with a stream had no frame left in a feed that others still decode
    worst: float = 0.0
    trace: list = field(default_factory=list)  # (parents, emitted) of every step


def run_streams(engine, sc, logits_fn, score_ok, compare_every_step=False):
    """-> Outcome.  score_ok(got, want, rounds, ref) -> bool."""
    K, S, N, E = sc.K, sc.S, sc.N, sc.E
    KR = 2 * K
    sj = sc.joint
    rng = np.random.default_rng(0)
    out = Outcome([FrameTracker(logits_fn, st.key, K, E, N, st.T, sc.blank, sc.ties_allowed) for st in sc.streams],
                  [None] * len(sc.streams))
    owner = [None] * S  # the stream in a slot
    seqs = [()] * (S * KR)
    engine.begin()
    n_feeds = max(st.start + len(st.chunks) + len(st.after) for st in sc.streams)

    def compare(what):
        res = engine.results()
        hyps, lengths, scores, stable, frames, tstable = res
        assert hyps.shape == (S, K, N) and lengths.shape == scores.shape == (S, K) and stable.shape == (S,)
        for s in range(S):
            at = (what, "slot", s)
            beam = [] if owner[s] is None else out.refs[owner[s]].open()
            for k in range(K):
                if k >= len(beam):
                    assert lengths[s, k] == 0 and scores[s, k] == -math.inf and not hyps[s, k].any(), (at, k, "empty")
                    assert frames is None or (frames[s, k] == -1).all(), (at, k, "empty frames")
                    continue
                y, sco, fr = beam[k]
                L = len(y)
                assert lengths[s, k] == L and hyps[s, k, :L].tolist() == list(y) and not hyps[s, k, L:].any(), (at, k, "ids")
                if frames is not None:
                    assert frames[s, k, :L].tolist() == list(fr) and (frames[s, k, L:] == -1).all(), (at, k, "frames", frames[s, k, :L], fr)
                assert seqs[s * KR + k] == y, (at, k, "the caller's sequence")
                ref = out.refs[owner[s]].ref
                assert score_ok(float(scores[s, k]), sco, ref.k, ref), (at, k, "score", float(scores[s, k]), sco)
                out.worst = max(out.worst, abs(float(scores[s, k]) - sco))
            want = 0 if owner[s] is None else out.refs[owner[s]].stable()
            assert stable[s] == want, (at, "stable", int(stable[s]), want)
            if tstable is not None:
                want_t = 0 if owner[s] is None else out.refs[owner[s]].timed_stable()
                assert tstable[s] == want_t <= stable[s], (at, "timed stable", int(tstable[s]), want_t)
            if owner[s] is not None:
                out.results[owner[s]] = tuple(None if x is None else np.array(x[s]).copy() for x in res)

    for f in range(n_feeds):
        fr, rs, fi = [0] * S, [0] * S, [0] * S
        left = [0] * S  # the frames of this feed a slot's stream will decode
        for n, st in enumerate(sc.streams):
            k = f - st.start
            if k == 0:
                owner[st.slot], rs[st.slot] = n, 1
                seqs[st.slot * KR: st.slot * KR + KR] = [()] * KR
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
        for step in range(Te * (E + 1)):
            rows = np.full((S * KR, sj.J), np.nan, np.float32)
            live = [s for s in range(S) if left[s] > 0]
            for s in live:
                tr, st = out.refs[owner[s]], sc.streams[owner[s]]
                for k in range(len(tr.ref.open[0])):
                    rows[s * KR + k] = sj.pred_rows(sc.script(st.key, tr.frame, seqs[s * KR + k]))[0]
            parents, emitted = engine.step(rows)
            out.steps += 1
            out.trace.append((np.array(parents).copy(), np.array(emitted).copy()))
            want_p, want_e = list(range(S * KR)), [-1] * (S * KR)
            for s in range(S):
                if s not in live:
                    out.frozen_steps += owner[s] is not None and bool(live)
                    continue
                tr = out.refs[owner[s]]
                p, e = tr.step()
                want_p[s * KR: s * KR + KR] = [s * KR + x for x in p]
                want_e[s * KR: s * KR + KR] = e
                if step % (E + 1) == E:
                    left[s] -= 1
            assert parents.tolist() == want_p, (f, step, "parents", parents.tolist(), want_p)
            assert emitted.tolist() == want_e, (f, step, "emitted", emitted.tolist(), want_e)
            seqs = [seqs[p] + ((e,) if e >= 0 else ()) for p, e in zip(parents.tolist(), emitted.tolist())]
            if compare_every_step or step % (E + 1) == E:
                compare(("feed", f, "step", step))
    for n, st in enumerate(sc.streams):
        if sum(st.chunks) == st.T and owner[st.slot] == n:
            assert out.refs[n].done, (n, "the stream was not decoded to its end")
    return out


def same_bits(a, b) -> bool:
    """Two streams' results, bit for bit (scores as bits)."""
    return all((x is None and y is None) or (x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()) for x, y in zip(a, b))


def check_expectations(sc, out):
    total = {}
    for tr in out.refs:
        for key in sc.expect:
            got = getattr(tr, key) if hasattr(tr, key) else getattr(tr.ref.ev, key)
            total[key] = total.get(key, 0) + (len(got) if isinstance(got, list) else got)
    for key, want in sc.expect.items():
        assert total[key] >= want, (sc.name, key, total[key], want)


def describe(sc, out):
    ev = [tr.ref.ev for tr in out.refs]
    return (f"{sc.name}: feeds={out.feeds} steps={out.steps} frozen={out.frozen_steps} merges={sum(e.closed_merges for e in ev)} "
            f"frame-merges={sum(t.frame_merges for t in out.refs)}/{sum(t.frame_merges_reported for t in out.refs)} "
            f"overflows={sum(e.overflows for e in ev)} ties={sum(e.ties for e in ev)} capped={sum(e.capped for e in ev)} "
            f"skipped={sum(e.skipped_closings for e in ev)} empty turns={sum(len(e.empty_turns) for e in ev)} "
            f"min gap={min(e.min_gap for e in ev):.3e} worst score error={out.worst:.3e}")


# ---------------------------------------------------------------------------------------------
# scenarios.  The seeds were picked on the restatement alone: every run checks the restatement's precondition (adjacent ranked
# entries are declared ties or more than twice the score bar apart) and the events a scenario expects.
# ---------------------------------------------------------------------------------------------
T13 = 13
CHUNKINGS = {"one": [13], "ones": [1] * 13, "zeros-between": [2, 0, 3, 0, 0, 1, 7], "cuts": [3, 1, 4, 5], "empty-final": [6, 7, 0]}
SPREAD = 3.0  # ds.random_script, blank 0: three utterances of 13 frames
SEEDS = {(0, 6): 16, (0, 12): 14, (1, 12): 7, (1, 130): 9}  # (joint_dtype, V) -> random_script's seed
GEOMETRY_SEEDS = {(0, 12, 1, 8): 22, (0, 12, 4, 2): 35, (0, 12, 1, 3): 23, (0, 12, 16, 1): 21, (1, 12, 4, 2): 25,
                  (1, 130, 4, 3): 18}  # (joint_dtype, V, K, E) -> seq_script's seed


def _script(dtype, V=None):
    V = V or (6 if dtype == 0 else 12)
    return V, ds.random_script(SEEDS.get((dtype, V), 3), V, spread=SPREAD, blank=0)


def chunking_scenario(name, K=4, E=2, dtype=0, slot=0, S=1, N=None, Tc=T13, V=None, J=0, chunks=None):
    """One stream of 13 frames through CHUNKINGS[name] (or `chunks`)."""
    V, script = _script(dtype, V)
    return Scenario(f"chunks-{name}-K{K}-E{E}-dt{dtype}-S{S}.{slot}", dtype, V, K, E, S, Tc, N or T13 * E, 0, script,
                    [Stream(slot, 0, T13, list(chunks or CHUNKINGS[name]))], J=J)


def frame_merge_scenario(K=4, E=2, dtype=0, V=None, J=0):
    """Closings merged into entries whose frames differ: one sequence reached as L + r tokens (L before the frame, r in it) by one
    path and as (L - 1) + (r + 1) by another.  The entry keeps its own frame row, and some such entries reach list A."""
    sc = chunking_scenario("cuts", K, E, dtype, V=V, J=J)
    sc.name = f"frame-merge-K{K}-E{E}-dt{dtype}-V{sc.V}"
    sc.expect = dict(closed_merges=4, frame_merges=2, frame_merges_reported=1)
    return sc


def overflow_frames(sc, logits_fn):
    """The frames of sc's first stream in which the closed list was longer than K before the cut (on the restatement alone)."""
    st = sc.streams[0]
    tr = FrameTracker(logits_fn, st.key, sc.K, sc.E, sc.N, st.T, sc.blank, sc.ties_allowed)
    frames = []
    for t in range(st.T):
        before = tr.ref.ev.overflows
        for _ in range(sc.E + 1):
            tr.step()
        if tr.ref.ev.overflows > before:
            frames.append(t)
    return frames


def overflow_boundary_scenario(logits_fn_of, K=4, E=2, dtype=0, V=None, J=0):
    """A chunk boundary directly after a frame whose closed list overflowed K (the frame is found on the restatement)."""
    sc = chunking_scenario("one", K, E, dtype, V=V, J=J)
    over = [t for t in overflow_frames(sc, logits_fn_of(sc)) if t + 1 < T13]
    assert over, "no frame's closed list overflows: the scenario shows nothing"
    cut = over[0] + 1
    sc.streams[0].chunks = [cut, T13 - cut]
    sc.name = f"overflow-boundary-{cut}-K{K}-E{E}-dt{dtype}"
    sc.expect = dict(overflows=1)
    return sc


def slots_scenario(slot, S=4, K=4, E=2, dtype=0, V=None, J=0):
    """The stream of chunking_scenario (key 0, chunks 3 1 4 5) in `slot`, beside streams that are reset, finished and fed other
    lengths in the same feeds (slots whose chunk is shorter freeze mid-feed); one of them is abandoned by a restart, one is fed
    after it finished."""
    V, script = _script(dtype, V)
    others = [s for s in range(S) if s != slot]
    streams = [Stream(slot, 0, T13, CHUNKINGS["cuts"], start=1)]
    streams.append(Stream(others[0], 1, T13, [5, 0, 2, 6], start=0, after=[3]))
    streams.append(Stream(others[1], 2, T13, [1, 1, 2, 9], start=0))           # abandoned after 2 frames ...
    streams.append(Stream(others[1], 1, T13, [7, 6], start=2, after=[2]))      # ... by this restart
    if len(others) > 2:
        streams.append(Stream(others[2], 2, T13, [13], start=2))
    return Scenario(f"slots-{slot}of{S}-K{K}-E{E}-dt{dtype}-V{V}", dtype, V, K, E, S, T13, T13 * E, 0, script, streams, J=J)


def final_scenario(K=4, E=2, dtype=0, V=None, J=0):
    """A final chunk that cuts a stream short (9 of 13 frames), frames fed to the finished slot, and a reset that reuses it for the
    whole utterance; beside it a stream in 2-frame chunks."""
    V, script = _script(dtype, V)
    streams = [Stream(0, 0, 9, [4, 5], start=0, after=[3, 2]), Stream(0, 0, T13, [13], start=4), Stream(1, 1, T13, [2, 2, 2, 2, 5], start=0)]
    return Scenario(f"final-K{K}-E{E}-dt{dtype}-V{V}", dtype, V, K, E, 2, T13, T13 * E, 0, script, streams, J=J)


def capacity_scenario(N, K=3, E=2, dtype=0):
    """max_hyp_len reached: hypotheses of N tokens offer no expansion and go on closing (mc's full-rows script)."""
    streams = [Stream(0, 0, 4, [1, 2, 1]), Stream(1, 1, 4, [4])]
    return Scenario(f"capacity-N{N}-K{K}-E{E}-dt{dtype}", dtype, 5, K, E, 2, 4, N, 4, mc.seq_script(8, 5, 2.0, 4, -3.0), streams,
                    expect=dict(capped=4))


def empty_turn_scenario(K=3, E=2, dtype=0):
    """Frame 2 of utterance 1 is a row of NaN for every hypothesis: nothing closes, the closed list is empty at the turn and the
    beam stays empty until the slot's reset, which starts utterance 0 in it."""
    script = mc.nan_for(ds.random_script(1, 7, spread=3.0, blank=0), 7, lambda b, t, y: b == 1 and t == 2)
    streams = [Stream(0, 1, 5, [2, 2, 1]), Stream(0, 0, 5, [3, 2], start=4), Stream(1, 2, 4, [4], start=1)]
    return Scenario(f"empty-turn-K{K}-E{E}-dt{dtype}", dtype, 7, K, E, 2, 4, 5 * E, 0, script, streams, expect=dict(empty_turns=3))


def nan_rows_scenario(K=3, E=2, dtype=0):
    """A NaN row for one hypothesis alone (utterance 0, frame 1, the hypotheses of one token): its closing is skipped."""
    script = mc.nan_for(ds.random_script(1, 7, spread=3.0, blank=0), 7, lambda b, t, y: b == 0 and t == 1 and len(y) == 1)
    return Scenario(f"nan-rows-K{K}-E{E}-dt{dtype}", dtype, 7, K, E, 1, 3, 5 * E, 0, script, [Stream(0, 0, 5, [1, 1, 3])],
                    expect=dict(skipped_closings=1))


def ties_scenario(K=4, E=2, dtype=0):
    """Declared exact ties (ds.tie_script): candidates by (hypothesis, symbol), closed entries by their place in the list."""
    V, p, q, blank = (9, 3, 6, 0) if dtype == 0 else (128, 5, 40, 4)
    streams = [Stream(0, 0, 5, [2, 0, 3]), Stream(1, 1, 6, [1, 5])]
    return Scenario(f"ties-K{K}-E{E}-dt{dtype}", dtype, V, K, E, 2, 5, 6 * E, blank, ds.tie_script(V, p, q, blank), streams,
                    ties_allowed=True, expect=dict(ties=6))


def geometry_scenario(S, K, slot, E=2, dtype=0, V=None, J=0, T=4, chunks=(1, 2, 1), Tc=None, blank=0):
    """One short stream in `slot` of S (rows S 2K: the smallest, one full 32-row tile, across its edge, several tiles) beside a
    second one in the last slot."""
    V = V or (12 if dtype else 6)
    script = mc.seq_script(GEOMETRY_SEEDS.get((dtype, V, K, E), 5), V, 3.0, blank, 1.5)
    streams = [Stream(slot, 0, T, list(chunks))]
    if S > 1:
        streams.append(Stream(S - 1 if slot != S - 1 else 0, 1, T, [T] if (Tc or T) >= T else [1] * T, start=1))
    return Scenario(f"geometry-S{S}-K{K}-E{E}-V{V}-dt{dtype}", dtype, V, K, E, S, Tc or T, T * E, blank, script, streams, J=J)


def k16_scenario(E=3, dtype=0):
    """Beam 16 at E = 3 over a script whose rows depend on the whole sequence (16 hypotheses of one shared row crowd together)."""
    return Scenario(f"chunks-cuts-K16-E{E}-dt{dtype}", dtype, 6, 16, E, 1, 3, 6 * E, 0, mc.seq_script(K16_SEED, 6, 3.0, 0, 1.5),
                    [Stream(0, 0, 6, [3, 1, 2])])


K16_SEED = 11


def cpu_scenarios(logits_fn_of):
    """name -> Scenario: everything the CPU mirror runs (the GPU file runs a part of it on each joint)."""
    out = [chunking_scenario(name) for name in CHUNKINGS]
    out += [frame_merge_scenario(), overflow_boundary_scenario(logits_fn_of)]
    out += [slots_scenario(slot) for slot in range(4)]
    out += [final_scenario(), capacity_scenario(3), capacity_scenario(1), empty_turn_scenario(), nan_rows_scenario(), ties_scenario()]
    out += [chunking_scenario("cuts", K=1, E=1), k16_scenario(),
            chunking_scenario("ones", K=2, E=8, Tc=1)]
    return {sc.name: sc for sc in out}
