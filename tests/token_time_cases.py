"""Helpers for the token-time tests (a helper module, not a conftest): float64 restatements of both decoders that also record
(frame, log-probability) per token, written from the "timed decoding" text of include/rnnt.h on top of the restatements of
tests/decode_scripts.py; the comparison of an engine's frames / log-probabilities with them; and a scripted beam whose
hypotheses share tokens but not frames.

Rules restated here:
  emission frame   the frame t whose joint evaluation appended the token (streams: counted from the reset);
  log-probability  logit[v] - lse of that decision, float64;
  merges           the first-ranked member of a group of identical sequences keeps its own pairs, the score is the logaddexp;
  timed stable     the longest prefix on which all hypotheses of a beam agree in token and frame.
Bars: frames exactly; a log-probability within decode_scripts.score_bar(1, max |lse|, logp): one decision's logsumexp bar plus
the f32 rounding of the stored value."""
import math

import numpy as np

from tests import decode_scripts as ds


class TimedBeamRestatement(ds.BeamRestatement):
    """BeamRestatement plus self.times[b][k]: the ((frame, logp), ...) of hypothesis k of utterance b."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.times = [[()] for _ in range(self.B)]

    def step(self):
        K, t = self.K, self.t
        before = [list(b) for b in self.beams]
        parents, emitted = super().step()
        for b in range(self.B):
            if t >= self.Tb[b] or (b, t) in self.ev.carried:
                continue
            new = []
            for k in range(len(self.beams[b])):
                i, v = parents[b * K + k] - b * K, emitted[b * K + k]
                row = self.times[b][i]
                if v >= 0:  # the survivor's own decision: parent i emitted v at this frame
                    lg = np.asarray(self.fn(b, t, before[b][i][0]), np.float64)
                    row = row + ((t, float(lg[v]) - ds._logsumexp(lg)),)
                new.append(row)
                assert len(row) == len(self.beams[b][k][0])
            self.times[b] = new
        return parents, emitted

    def timed_stable(self, b):
        rows, toks = self.times[b], [y for y, _ in self.beams[b]]
        return timed_common_prefix(toks, [[f for f, _ in r] for r in rows])


def timed_common_prefix(tokens, frames):
    """tokens / frames: per occupied hypothesis its token list and frame list -> the prefix agreeing in both."""
    if not tokens:
        return 0
    n = 0
    while all(n < len(y) for y in tokens) and all(y[n] == tokens[0][n] and f[n] == frames[0][n] for y, f in zip(tokens, frames)):
        n += 1
    return n


class TimedGreedyRestatement(ds.GreedyRestatement):
    """GreedyRestatement plus self.times[b]: the ((frame, logp), ...) of row b."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.times = [()] * self.B

    def step(self, max_hyp_len):
        at = [(self.t[b], self.y[b]) for b in range(self.B)]
        emitted, all_done = super().step(max_hyp_len)
        for b, v in enumerate(emitted):
            if v >= 0:
                lg = np.asarray(self.fn(b, at[b][0], at[b][1]), np.float64)
                self.times[b] = self.times[b] + ((at[b][0], float(lg[v]) - ds._logsumexp(lg)),)
        return emitted, all_done


def restate_beam(sc, logits_fn):
    ref = TimedBeamRestatement(logits_fn, sc.B, sc.K, sc.frames, sc.maxT, sc.blank, sc.ties_allowed)
    for _ in range(sc.steps):
        ref.step()
    return ref


def restate_greedy(sc, logits_fn):
    ref = TimedGreedyRestatement(logits_fn, sc.B, sc.frames, sc.max_symbols, sc.max_per_frame, sc.maxT, sc.blank, sc.ties_allowed)
    lens = list(sc.hyp_lens)
    N = lens.pop(0)
    for _ in range(100000):
        _, d = ref.step(N)
        if d == 0:
            continue
        if d == 2 and lens:
            N = lens.pop(0)
            continue
        return ref
    raise AssertionError("the scripted decode did not end")


def check_row(frames, logp, want, max_lse, what):
    """One hypothesis: frames / logp arrays (padded) against want = ((frame, logp), ...).  -> worst (error, bar), printed by the
    callers before anything is asserted on the log-probabilities."""
    n = len(want)
    assert frames[:n].tolist() == [f for f, _ in want], (what, "frames", frames[:n].tolist(), [f for f, _ in want])
    assert (frames[n:] == -1).all() and not np.asarray(logp[n:]).any(), (what, "padding: -1 and 0")
    worst = (0.0, 0.0)
    for j, (_, lp) in enumerate(want):
        err, bar = abs(float(logp[j]) - lp), ds.score_bar(1, max_lse, lp)
        if err >= worst[0]:
            worst = (err, bar)
        assert err <= bar, (what, j, float(logp[j]), lp, err, bar)
    return worst


def check_beam_times(sc, ref, lengths, frames, logp):
    worst = (0.0, 0.0)
    for b in range(sc.B):
        for k in range(sc.K):
            want = ref.times[b][k] if k < len(ref.beams[b]) else ()
            assert lengths[b, k] == len(want), (b, k)
            worst = max(worst, check_row(frames[b, k], logp[b, k], want, ref.ev.max_lse, (sc.name, b, k)))
    return worst


def check_greedy_times(sc, ref, frames, logp):
    worst = (0.0, 0.0)
    for b in range(sc.B):
        worst = max(worst, check_row(frames[b], logp[b], ref.times[b], ref.ev.max_lse, (sc.name, b)))
    return worst


# ---- a beam whose hypotheses share tokens but not frames ---------------------------------------------------------------------
def late_twin_script(V, blank, a=1, c=2, d=3, e=4):
    """K = 3, one utterance.  Frame 0: the blank leads, `a` 0.4 behind -> the beam holds () and (a) (and a stray far below).
    Frame 1: () emits `a`, (a) takes the blank: two taken candidates with the sequence (a) MERGE, and the first-ranked -- () + a,
    emitted at frame 1 -- survives; the third taken candidate is (a) + c of the frame-0 hypothesis.  Beam: (a) with frames (1),
    (a c) with frames (0, 1): one token shared, emitted at different frames, so stable_lengths is 1 and the timed stable length
    0.  Frames 2, 3: both lines go on with `d`.  From frame 4 on the (a c ...) line spreads its mass over the vocabulary and the
    first line offers three strong candidates: the beam is taken over by descendants of one hypothesis and the timed stable
    length catches up with stable_lengths.  The blank's level moves with the frame so that no two paths add up alike."""
    def script(b, t, y):
        L = -9.0 - 0.2 * np.arange(V)
        low = -6.0 - 0.37 * t
        if t == 0:
            L[blank], L[a] = 0.0, -0.4
        elif t == 1:
            if y == ():
                L[a], L[blank] = 0.0, -3.0
            elif y == (a,):
                L[blank], L[c] = -0.5, -0.7
        elif len(y) >= 2 and y[1] == c:
            if t < 4:
                L[d], L[blank] = -0.9, low
            else:
                L = -0.3 * np.arange(V) - 0.01 * t
        elif t < 4:
            L[d], L[blank] = 0.0, low
        else:
            L[d], L[blank], L[e] = 0.0, -1.5 - 0.01 * t, -1.9
        return L

    return script


def late_twin_scenario():
    V = 9
    return ds.BeamScenario("late-twin", 0, V, 1, 3, 7, [7], 0, late_twin_script(V, 0), 7)


# ---- streams: a schedule of chunked feeds over the slots of one decoder ------------------------------------------------------
def run_streams(dec, streams, plans, read, seed=0, extra_restart=None, after_feed=None):
    """Feed streams through `dec` (a StreamingGreedyDecoder or StreamingBeamDecoder).  plans[i] = (slot, start_feed, chunk
    lengths): a stream starts at its start feed and takes one chunk per feed, sitting a feed out now and then, beside the other
    streams' traffic.  extra_restart = (feed, slot): a start() in mid-run (of a slot whose stream then begins again elsewhere
    or never).  -> per stream read(dec, slot) right after its final feed.  after_feed(dec, owner) runs after every feed."""
    import random

    import torch

    rng = random.Random(seed)
    S, Tc, F = dec.S, dec.Tc, streams[0].shape[1]
    state = [dict(pos=0, k=0, started=False, done=False) for _ in streams]
    results, feed_no = {}, 0
    while not all(s["done"] for s in state):
        to_start = [i for i, (slot, sf, _) in enumerate(plans) if sf == feed_no]
        if to_start:
            dec.start([plans[i][0] for i in to_start])
            for i in to_start:
                state[i]["started"] = True
        if extra_restart is not None and extra_restart[0] == feed_no:
            dec.start([extra_restart[1]])
        mel = torch.randn(S, Tc, F, dtype=streams[0].dtype, device=streams[0].device)  # (garbage past each slot's frames)
        frames, final, owner = [0] * S, [False] * S, {}
        for i, (slot, _, chunks) in enumerate(plans):
            st = state[i]
            if not st["started"] or st["done"] or (feed_no % 3 == 1 and rng.random() < 0.5):
                continue
            c = chunks[st["k"]]
            mel[slot, :c] = streams[i][st["pos"]: st["pos"] + c]
            frames[slot], final[slot] = c, st["k"] == len(chunks) - 1
            owner[slot] = i
            st["pos"] += c
            st["k"] += 1
        dec.feed(mel, frames, final)
        if after_feed is not None:
            after_feed(dec, owner)
        for slot, i in owner.items():
            if final[slot]:
                state[i]["done"] = True
                results[i] = read(dec, slot)
        feed_no += 1
    return results


def read_timed_greedy(dec, slot):
    """-> (ids, frames, logp bits, score bits) of one slot, as host data that compares bitwise."""
    ids, frames, logp = dec.timed_hypotheses()
    _, n, scores = dec.hypotheses()
    n = int(n[slot])
    assert (frames[slot, n:] == -1).all() and not logp[slot, n:].any() and not ids[slot, n:].any()
    return (ids[slot, :n].tolist(), frames[slot, :n].tolist(), logp[slot, :n].cpu().numpy().tobytes(),
            scores[slot].cpu().numpy().tobytes())


def read_timed_beam(dec, slot):
    """-> per occupied hypothesis (ids, frames, logp bits, score bits), then (stable, timed stable) of one slot."""
    ids, lengths, scores, frames, logp = dec.timed_nbest()
    stable, tstable = int(dec.bj.results()[3][slot]), int(dec.timed_stable_lengths()[slot])
    rows = []
    for k in range(dec.K):
        n = int(lengths[slot, k])
        assert (frames[slot, k, n:] == -1).all() and not logp[slot, k, n:].any() and not ids[slot, k, n:].any()
        if math.isfinite(float(scores[slot, k])):
            rows.append((ids[slot, k, :n].tolist(), frames[slot, k, :n].tolist(), logp[slot, k, :n].cpu().numpy().tobytes(),
                         scores[slot, k].cpu().numpy().tobytes()))
    assert tstable == timed_common_prefix([r[0] for r in rows], [r[1] for r in rows]) and tstable <= stable
    return rows, stable, tstable
