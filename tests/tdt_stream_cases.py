"""Streaming greedy TDT decoding over slots (include/rnnt_tdt_stream.h): scenarios and the driver that plays the caller (a helper
module, not a conftest).  The reference is tests/tdt_decode_cases.TDTRestatement on each stream's WHOLE utterance: chunking, slots
and restarts exist on the decoder's side alone.

A Scenario holds streams; a stream lives in a slot from its `start` feed on and brings chunks[k] frames at feed start + k, with the
final flag on its last chunk.  A later stream in the same slot restarts the slot (the earlier one is abandoned where it stands).
run_streams feeds them, steps the decoder until its all-done word is 1 after every feed, and holds it against the restatements at
every feed and step: emitted, all_done, lengths, ids and frames (since the slot's reset) exactly; scores and log-probabilities within
the bars the calling test passes.  It picks the pred_proj row of a slot from the restatement's (stream, absolute frame, tokens).

An engine has begin(max_hyp_len), feed(enc [S, Te, H] or None, frames, reset, final, max_symbols or None) -> (lengths, scores,
all_done), step(rows [S, J]) -> (emitted, all_done, lengths, scores, hyps, frames, logp) and grow(max_hyp_len); all numpy."""
import math
from dataclasses import dataclass, field

import numpy as np

from tests.tdt_decode_cases import TDTRestatement, head_script

NO_BUDGET = 2**31 - 1
CHUNKINGS = {"one": [13], "ones": [1] * 13, "ragged": [2, 0, 3, 1, 7], "final-on-empty": [5, 8, 0]}  # T = 13


@dataclass
class Stream:
    slot: int
    key: int  # the `b` its script sees: streams with one key have one utterance
    T: int
    chunks: list
    start: int = 0
    max_symbols: object = None


@dataclass
class Scenario:
    name: str
    V: int
    durations: list
    S: int
    Tc: int
    cap: int
    blank: int
    script: object  # (key, absolute frame, tokens) -> [V + D] float64 logits
    streams: list
    hyp_lens: list = field(default_factory=lambda: [64])
    tail_feeds: int = 0  # feeds without frames after the last chunk

    @property
    def R(self):
        return self.V + len(self.durations)


@dataclass
class Outcome:
    refs: list
    results: list    # per stream: (ids, frames, logp, length, score) as the decoder last reported them while the stream owned its slot
    idle_feeds: list  # per stream: feeds that brought it frames while it sat on a carry
    feeds: int = 0
    steps: int = 0
    paused_steps: int = 0
    worst_score: float = 0.0
    worst_score_bar: float = 0.0
    worst_logp: float = 0.0
    worst_logp_bar: float = 0.0


def run_streams(engine, sc, logits_fn, pred_row, enc_rows, score_bar, logp_bar, ties_allowed=False, min_gap=1e-6, check=True):
    """logits_fn(key, t, tokens) -> the restatement's logits; pred_row(key, t, tokens) -> [J]; enc_rows(key, t0, count) -> [count, H]."""
    S, V = sc.S, sc.V
    refs = [TDTRestatement(lambda b, t, y, k=st.key: logits_fn(k, t, y), 1, V, sc.durations, [st.T],
                           None if st.max_symbols is None else [st.max_symbols], sc.cap, st.T, sc.blank, ties_allowed, min_gap)
            for st in sc.streams]
    out = Outcome(refs, [None] * len(sc.streams), [0] * len(sc.streams))
    budgets = any(st.max_symbols is not None for st in sc.streams)
    hyp_lens = list(sc.hyp_lens)
    N = hyp_lens.pop(0)
    engine.begin(N)
    owner, avail, restarted = [None] * S, [0] * S, [False] * S
    waiting = lambda s: owner[s] is not None and not refs[owner[s]].done[0] and refs[owner[s]].t[0] < avail[s]  # noqa: E731
    blank_row = np.full_like(np.asarray(pred_row(sc.streams[0].key, 0, ())), np.nan)  # (slots that do not run read nothing)

    def compare(at, lengths, scores, hyps=None, frames=None, logp=None):
        for s in range(S):
            i = owner[s]
            if i is None:
                assert lengths[s] == 0, (at, s, "a slot that never started")
                continue
            ref = refs[i]
            n = len(ref.y[0])
            assert lengths[s] == n, (at, s, "length", int(lengths[s]), n)
            want = ref.score[0]
            if want != want:
                assert scores[s] != scores[s], (at, s, "the score must be NaN")
            else:
                err, bar = abs(float(scores[s]) - want), score_bar(ref.steps[0], ref.ev.max_lse, want)
                assert err <= bar, (at, s, "score", float(scores[s]), want, err, bar)
                if err >= out.worst_score:
                    out.worst_score, out.worst_score_bar = err, bar
            if hyps is None:
                continue
            assert hyps[s, :n].tolist() == list(ref.y[0]), (at, s, "ids")
            assert frames[s, :n].tolist() == list(ref.frames[0]), (at, s, "frames", frames[s, :n].tolist(), list(ref.frames[0]))
            if not restarted[s]:
                assert not hyps[s, n:].any() and (frames[s, n:] == -1).all() and not logp[s, n:].any(), (at, s, "nothing else is written")
            for j, lp in enumerate(ref.logp[0]):
                if lp != lp:
                    assert logp[s, j] != logp[s, j], (at, s, j, "the log-probability must be NaN")
                    continue
                err, bar = abs(float(logp[s, j]) - lp), logp_bar(ref.ev.max_lse, lp)
                assert err <= bar, (at, s, j, "logp", float(logp[s, j]), lp, err, bar)
                if err >= out.worst_logp:
                    out.worst_logp, out.worst_logp_bar = err, bar
            out.results[i] = (hyps[s, :n].copy(), frames[s, :n].copy(), logp[s, :n].copy(), int(lengths[s]), scores[s].copy())

    n_feeds = max(st.start + len(st.chunks) for st in sc.streams) + sc.tail_feeds
    for f in range(n_feeds):
        frames, reset, final, maxsym = [0] * S, [0] * S, [0] * S, [NO_BUDGET] * S
        for i, st in enumerate(sc.streams):
            if st.start == f:
                restarted[st.slot] = owner[st.slot] is not None
                owner[st.slot], avail[st.slot], reset[st.slot] = i, 0, 1
                if st.max_symbols is not None:
                    maxsym[st.slot] = st.max_symbols
        chunk = {}
        for s in range(S):
            if owner[s] is None:
                continue
            st = sc.streams[owner[s]]
            k = f - st.start
            if 0 <= k < len(st.chunks):
                frames[s], final[s] = st.chunks[k], int(k == len(st.chunks) - 1)
                chunk[s] = (st.key, avail[s], st.chunks[k])
                avail[s] += st.chunks[k]
        Te = max(frames)
        enc = None
        if Te > 0:
            for s, (key, t0, c) in chunk.items():
                if c > 0:
                    rows = np.asarray(enc_rows(key, t0, c))
                    if enc is None:
                        enc = np.full((S, Te, rows.shape[1]), np.nan, rows.dtype)  # (NaN past each slot's frames: never read)
                    enc[s, :c] = rows
        lengths, scores, all_done = engine.feed(enc, frames, reset, final, maxsym if budgets else None)
        out.feeds += 1
        for s in chunk:
            out.idle_feeds[owner[s]] += frames[s] > 0 and not refs[owner[s]].done[0] and not waiting(s)
        if check:
            compare((f, "feed"), lengths, scores)
            assert int(all_done) == (0 if any(waiting(s) for s in range(S)) else 1), (f, "all_done after the feed", int(all_done))
        flag, last = int(all_done), None
        while True:  # (one more step than needed: a step on slots that are all done changes nothing)
            live = [s for s in range(S) if waiting(s) and refs[owner[s]].runs(0, N)]
            row = {s: np.asarray(pred_row(sc.streams[owner[s]].key, refs[owner[s]].t[0], refs[owner[s]].y[0])) for s in live}
            rows = np.stack([row.get(s, blank_row) for s in range(S)])
            res = engine.step(rows)
            emitted, all_done, lengths, scores, hyps, hfr, hlp = res
            out.steps += 1
            want_e = [-1] * S
            for s in live:
                want_e[s] = refs[owner[s]].step(N)[0][0]
            running = any(waiting(s) and len(refs[owner[s]].y[0]) < N for s in range(S))
            paused = any(waiting(s) and len(refs[owner[s]].y[0]) >= N for s in range(S))
            want_d = 0 if running else (2 if paused else 1)
            out.paused_steps += want_d == 2
            if check:
                at = (f, out.steps)
                assert emitted.tolist() == want_e, (at, "emitted", emitted.tolist(), want_e)
                assert int(all_done) == want_d, (at, "all_done", int(all_done), want_d)
                compare(at, lengths, scores, hyps, hfr, hlp)
            if flag == 1:  # that was the extra step
                assert not live and (last is None or all(np.array_equal(p, q, equal_nan=True) for p, q in zip(last[2:], res[2:])))
                break
            flag, last = want_d, res
            if want_d == 2:
                assert hyp_lens, "the scenario pauses more often than it has buffers"
                N = hyp_lens.pop(0)
                engine.grow(N)
                flag = 0
    return out


# ---------------------------------------------------------------------------------------------
# scenarios: scripted logits (the wanted token and duration index at logit 0, the others 0.5 apart below)
# ---------------------------------------------------------------------------------------------
def chunking_scenario(durations, V=9, blank=0):
    """One utterance of 13 frames in four slots at once, through the four chunkings; each slot starts one feed after the last, so the
    slots are in different phases all the time."""
    streams = [Stream(s, 0, 13, list(c), start=s) for s, c in enumerate(CHUNKINGS.values())]
    return Scenario(f"chunkings-{durations}", V, list(durations), 4, 13, 3, blank,
                    head_script(len(durations) * 17 + durations[-1], V, durations, blank), streams)


def carry_scenario():
    """Durations [0, 1, 2, 4], d = 1 except: a jump of 4 from frame 2 (fed as 1-frame chunks: it lands 3 frames past its chunk and the
    slot idles for three feeds), and a jump of 4 from the last frame 12 (dropped by the final chunk).  Slot 1 gets the same utterance
    as [5, 8]: there the first jump stays inside its chunk."""
    V, dur = 8, [0, 1, 2, 4]
    dur_of = lambda b, t, y: 3 if t in (2, 12) else 1  # noqa: E731
    tok_of = lambda b, t, y: 1 + (t % (V - 1)) if t in (2, 12) else None  # noqa: E731  (tokens on both jumps)
    return Scenario("carry", V, dur, 2, 13, 2, 0, head_script(31, V, dur, 0, dur_of=dur_of, tok_of=tok_of),
                    [Stream(0, 0, 13, [1] * 13), Stream(1, 0, 13, [5, 8])])


def cap_at_chunk_end_scenario():
    """Durations [0, 1, 2], cap 3: on frame 3, the last of the chunk [4], every decision is a token with d = 0 until the cap moves the
    slot on, into the next chunk; on frame 7 a blank with d = 0."""
    V, dur = 7, [0, 1, 2]
    dur_of = lambda b, t, y: 0 if t in (3, 7) else 1  # noqa: E731
    tok_of = lambda b, t, y: (1 + len(y) % (V - 1)) if t == 3 else (0 if t == 7 else None)  # noqa: E731
    return Scenario("cap-at-chunk-end", V, dur, 1, 9, 3, 0, head_script(32, V, dur, 0, dur_of=dur_of, tok_of=tok_of),
                    [Stream(0, 0, 13, [4, 9])])


def budget_scenario():
    """A budget of 3 symbols spent inside the first chunk; two more chunks and an empty feed change nothing; then the slot is reset
    for another utterance (no budget), while slot 1 decodes its own all along."""
    V, dur = 8, [0, 1, 2]
    tok_of = lambda b, t, y: 1 + (t + len(y) + b) % (V - 1)  # noqa: E731  (never the blank)
    return Scenario("budget", V, dur, 2, 13, 2, 0, head_script(33, V, dur, 0, tok_of=tok_of, dur_of=lambda b, t, y: 1),
                    [Stream(0, 0, 13, [6, 3, 4, 0], max_symbols=3), Stream(0, 1, 13, [13], start=4), Stream(1, 2, 13, [3, 3, 3, 2, 2])])


def pause_scenario():
    """Tokens on every frame and buffers of 2, 4 and 32 (what doubling gives): the decode pauses inside a chunk (all_done = 2) and goes on when grown."""
    V, dur = 8, [0, 1, 2]
    tok_of = lambda b, t, y: 1 + (t + len(y) + b) % (V - 1)  # noqa: E731
    return Scenario("pause", V, dur, 2, 8, 2, 0, head_script(34, V, dur, 0, tok_of=tok_of),
                    [Stream(0, 0, 13, [8, 5]), Stream(1, 1, 13, [4, 4, 5], start=1)], hyp_lens=[2, 4, 32])


def phases_scenario():
    """Three slots in different phases; slot 1 is restarted with another utterance while its first one is half way and the others run."""
    V, dur = 9, [0, 1, 2, 3, 4]
    return Scenario("phases", V, dur, 3, 6, 3, 4, head_script(35, V, dur, 4),
                    [Stream(0, 0, 13, [6, 0, 6, 1]), Stream(1, 1, 13, [2, 2, 2, 2, 5], start=1), Stream(2, 2, 13, [1, 6, 6], start=2),
                     Stream(1, 3, 13, [3, 5, 5], start=3)], tail_feeds=1)


def nan_scenario():
    """A NaN logit row at (utterance 1, frame 4), inside its second chunk: blank, d = 1 and a NaN score for that slot alone."""
    V, dur = 8, [0, 1, 2]
    base = head_script(36, V, dur, 0)
    script = lambda b, t, y: np.full(V + len(dur), np.nan) if (b, t) == (1, 4) else base(b, t, y)  # noqa: E731
    return Scenario("nan-row", V, dur, 3, 13, 2, 0, script,
                    [Stream(0, 0, 13, [13]), Stream(1, 1, 13, [3, 10]), Stream(2, 2, 13, [7, 6])])


def scripted_pred_row(sc, J, c, dtype=np.float64):
    """W2 = c I: the pred_proj row whose logits are the script's (atanh(L / c) in the first V + D units)."""
    def row(key, t, y):
        L = np.asarray(sc.script(key, t, y), np.float64)
        out = np.zeros(J, dtype)
        with np.errstate(invalid="ignore"):
            out[: sc.R] = np.arctanh(L / c)
        return out
    return row


def describe(sc, out):
    evs = [r.ev for r in out.refs]
    tot = lambda name: sum(getattr(e, name) for e in evs)  # noqa: E731
    gap = min(e.min_gap for e in evs)
    return (f"[{sc.name}] feeds={out.feeds} steps={out.steps} paused-steps={out.paused_steps} idle-feeds={out.idle_feeds} "
            f"capped={tot('capped')} d0-chains={tot('zero_chains')} blank-d0={tot('blank_d0')} blanks={tot('blanks')} "
            f"jumps-past-end={tot('jumps_past_end')} no-finite-heads={tot('no_finite')} "
            f"durations-used={sorted(set().union(*(e.durations_used for e in evs)))} min-gap={'-' if gap == math.inf else f'{gap:.3g}'} "
            f"score-error={out.worst_score:.3e} bar={out.worst_score_bar:.3e} logp-error={out.worst_logp:.3e} bar={out.worst_logp_bar:.3e}")


# ---------------------------------------------------------------------------------------------
# a caller without a reference: the rows follow the tokens the decoder itself reports (a prediction network sees tokens, not frames)
# ---------------------------------------------------------------------------------------------
def free_run(engine, S, streams, pred_row, enc_rows, N=64, max_steps=400):
    """One stream per slot at most.  pred_row(key, tokens) -> [J].  -> ({stream index: (ids, frames or None, logp or None, length,
    score)} read after the last feed, the all-done word of every feed, steps taken)."""
    assert len({st.slot for st in streams}) == len(streams)
    engine.begin(N)
    by_slot = {st.slot: i for i, st in enumerate(streams)}
    avail, ys = [0] * S, [()] * S
    blank_row = np.full_like(np.asarray(pred_row(streams[0].key, ())), np.nan)
    feed_flags, steps, res = [], 0, None

    def step():
        rows = np.stack([np.asarray(pred_row(streams[by_slot[s]].key, ys[s])) if s in by_slot else blank_row for s in range(S)])
        out = engine.step(rows)
        for s in by_slot:
            ys[s] = tuple(int(v) for v in out[4][s, : out[2][s]])
        return out

    for f in range(max(st.start + len(st.chunks) for st in streams)):
        frames, reset, final = [0] * S, [0] * S, [0] * S
        enc = None
        chunk = {}
        for st in streams:
            k = f - st.start
            if k == 0:
                reset[st.slot] = 1
            if 0 <= k < len(st.chunks):
                frames[st.slot], final[st.slot] = st.chunks[k], int(k == len(st.chunks) - 1)
                chunk[st.slot] = (st.key, avail[st.slot], st.chunks[k])
                avail[st.slot] += st.chunks[k]
        Te = max(frames)
        for s, (key, t0, c) in chunk.items():
            if c > 0:
                rows = np.asarray(enc_rows(key, t0, c))
                if enc is None:
                    enc = np.full((S, Te, rows.shape[1]), np.nan, rows.dtype)
                enc[s, :c] = rows
        _, _, flag = engine.feed(enc, frames, reset, final, None)
        feed_flags.append(int(flag))
        while flag != 1:
            assert flag == 0 and steps < max_steps, (f, flag, steps)
            res = step()
            flag = res[1]
            steps += 1
    res = step()  # (every slot is done: this step changes nothing and reads the buffers)
    assert res[1] == 1 and (res[0] == -1).all()
    results = {}
    for s, i in by_slot.items():
        n = int(res[2][s])
        results[i] = (res[4][s, :n].copy(), None if res[5] is None else res[5][s, :n].copy(),
                      None if res[6] is None else res[6][s, :n].copy(), n, res[3][s].copy())
    return results, feed_flags, steps


def same_bits(a, b) -> bool:
    """Two results of free_run / run_streams, bit for bit (NaN payloads included)."""
    if len(a) != len(b):
        return False
    for p, q in zip(a, b):
        if (p is None) != (q is None):
            return False
        if p is not None:
            p, q = np.asarray(p), np.asarray(q)
            if p.shape != q.shape or p.dtype != q.dtype or p.tobytes() != q.tobytes():
                return False
    return True
