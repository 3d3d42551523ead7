"""CPU tests of streaming greedy TDT decoding (tdt.TDTGreedyStreamJoint, tdt.StreamingTDTGreedyDecoder,
StreamingTranscriber(tdt_durations=...)): the torch route in float64 against tests/tdt_decode_cases.TDTRestatement on each stream's
whole utterance.  The joint is scripted: W1 = 0, b1 = 0, W2 = c I, so the logits are c tanh(pred_proj) and tests/tdt_stream_cases.
run_streams picks the pred_proj row from the restatement's (stream, absolute frame, tokens).  ids, frames, lengths, emitted and
all_done are compared exactly at every feed and step, scores and log-probabilities to 1e-12."""
import types

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import decoding, tdt
from rnnt_speech_recognition_amd.decoding import StreamingTranscriber
from tests import frontend_cases as fc
from tests import tdt_stream_cases as cases
from tests.tdt_decode_cases import DURATION_SETS
from tests.test_frontend import small_model

C = 16.0
BAR = 1e-12


class TorchStreamEngine:
    """tdt.TDTGreedyStreamJoint on CPU tensors in float64, behind the numpy interface of run_streams."""

    def __init__(self, sc, H=3):
        R = sc.R
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)  # noqa: E731
        joint = types.SimpleNamespace(W1=z(H, R), b1=z(R), W2=C * torch.eye(R, dtype=torch.float64), b2=z(R), blank_label=sc.blank)
        self.sc, self.H = sc, H
        self.gj = tdt.TDTGreedyStreamJoint(joint, sc.durations)
        assert not self.gj.engine

    def begin(self, N):
        self.gj.begin(self.sc.S, self.sc.Tc, self.sc.cap, N, device="cpu")
        assert int(self.gj.all_done) == 1  # every slot finished

    def feed(self, enc, frames, reset, final, max_symbols):
        self.gj.feed(None if enc is None else torch.from_numpy(enc), frames, reset, final, max_symbols)
        return self.gj.lengths.numpy().copy(), self.gj.scores.numpy().copy(), int(self.gj.all_done)

    def step(self, rows):
        gj = self.gj
        emitted = gj.step(pred_proj=torch.from_numpy(rows))
        return (emitted.numpy().copy(), int(gj.all_done), gj.lengths.numpy().copy(), gj.scores.numpy().copy(), gj.hyps.numpy().copy(),
                gj.frames.numpy().copy(), gj.logp.numpy().copy())

    def grow(self, N):
        while self.gj.hyps.shape[1] < N:
            self.gj.grow_hyps()


def play(sc):
    eng = TorchStreamEngine(sc)
    out = cases.run_streams(eng, sc, sc.script, cases.scripted_pred_row(sc, sc.R, C), lambda key, t0, c: np.zeros((c, eng.H)),
                            lambda n, lse, s: BAR, lambda lse, lp: BAR)
    print(cases.describe(sc, out))
    return out


def same(a, b):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


@pytest.mark.parametrize("durations", DURATION_SETS, ids=str)
def test_every_chunking_ends_as_the_whole_utterance(durations):
    sc = cases.chunking_scenario(durations)
    out = play(sc)
    assert all(r.done[0] for r in out.refs) and sum(len(r.y[0]) for r in out.refs) >= 4
    for res in out.results[1:]:  # one utterance through four chunkings: one result, bit for bit (and run_streams held each to the restatement)
        assert same(res, out.results[0])


def test_a_jump_is_carried_over_three_feeds_and_dropped_by_the_final_chunk():
    sc = cases.carry_scenario()
    out = play(sc)
    assert out.idle_feeds == [3, 0]  # the jump of 4 from frame 2: 1-frame chunks 3, 4 and 5 find the slot on its carry
    for r in out.refs:
        assert 4 in r.ev.durations_used and r.ev.jumps_past_end >= 1 and r.ev.jumps_from_last >= 1 and r.done[0]
        assert 2 in r.frames[0] and 12 in r.frames[0] and not {3, 4, 5} & set(r.frames[0])
    assert same(out.results[0], out.results[1])


def test_a_zero_duration_chain_ended_by_the_cap_on_the_last_frame_of_a_chunk_and_a_blank_with_zero_duration():
    sc = cases.cap_at_chunk_end_scenario()
    out = play(sc)
    r = out.refs[0]
    assert r.ev.capped >= 1 and r.ev.zero_chains >= 2 and r.ev.blank_d0 >= 1
    assert list(r.frames[0]).count(3) == sc.cap and sc.streams[0].chunks[0] == 4  # frame 3 is the chunk's last
    assert 4 in r.frames[0] or r.t[0] > 4  # ... and the decode went on in the next chunk


def test_a_spent_budget_finishes_the_slot_until_its_reset():
    sc = cases.budget_scenario()
    out = play(sc)
    first, second, other = out.refs
    assert len(first.y[0]) == 3 and first.t[0] < 6, "the budget must be spent inside the first chunk"
    assert out.results[0][3] == 3
    assert second.done[0] and len(second.y[0]) > 3 and second.frames[0][0] == 0  # the reset slot counts frames from 0 again
    assert other.done[0] and out.results[2][3] == len(other.y[0])


def test_a_full_buffer_pauses_inside_a_chunk_and_grow_hyps_resumes():
    sc = cases.pause_scenario()
    out = play(sc)
    assert out.paused_steps >= 2 and all(r.done[0] for r in out.refs) and max(len(r.y[0]) for r in out.refs) > 5


def test_three_slots_in_different_phases_and_a_restart():
    sc = cases.phases_scenario()
    out = play(sc)
    a, b, c, b2 = out.refs
    assert a.done[0] and c.done[0] and b2.done[0]
    assert not b.done[0] and 0 < b.t[0] < 13, "slot 1 must be restarted half way through its first utterance"
    assert out.results[3][3] == len(b2.y[0]) > 0


def test_a_nan_row_costs_its_slot_alone():
    sc = cases.nan_scenario()
    out = play(sc)
    assert out.refs[1].ev.no_finite == 2 and np.isnan(out.results[1][4])
    assert np.isfinite(out.results[0][4]) and np.isfinite(out.results[2][4])


def test_begin_and_feed_check_their_arguments():
    sc = cases.carry_scenario()
    eng = TorchStreamEngine(sc)
    with pytest.raises(ValueError, match="max_per_frame"):
        eng.gj.begin(2, 4, 0, 8, device="cpu")
    eng.gj.begin(2, 4, 2, 8, device="cpu")
    with pytest.raises(ValueError, match="at most 4"):
        eng.gj.feed(torch.zeros(2, 5, 3, dtype=torch.float64), [5, 5])
    assert pkg.TDTGreedyStreamJoint is tdt.TDTGreedyStreamJoint and pkg.StreamingTDTGreedyDecoder is tdt.StreamingTDTGreedyDecoder


# ---------------------------------------------------------------------------------------------
# the decoder and the transcriber on a small model
# ---------------------------------------------------------------------------------------------
DUR = [0, 1, 2, 3, 4]


def small_tdt_stream_model(seed=3, V=11, H=64, J=64, scale=3.0, device="cpu", dtype=torch.float64):
    """A Transducer with H = J = 64 and reduction factor 2 whose joint has V + D columns, random weights.  Two encoder blocks with
    the time reduction between them: the streaming encoder (joint.EncoderStream) needs the reduction before the last block."""
    torch.manual_seed(seed)
    hp = pkg.HParams(vocab_size=V, mel_bins=4, downsample_factor=2, embedding_size=8, encoder_layers=2, encoder_size=H,
                     projection_size=H, time_reduction_index=0, pred_net_layers=1, pred_net_size=H, joint_net_size=J)
    model = pkg.Transducer(hp)
    model.joint = pkg.JointLoss(H, J, V + len(DUR))
    with torch.no_grad():
        model.joint.W2.mul_(scale)  # (wider logits: decisions with a margin)
        model.joint.b2.normal_(0.0, 0.5)
    return model.to(device=device, dtype=dtype).eval(), hp


def equal_results(got, want, bar=0.0):
    """(ids, frames, logp, length, score): ids, frames and length exactly; logp and score bitwise (bar 0), or within bar max(1, |x|)."""
    ids, frames, logp, n, score = (torch.as_tensor(v) for v in got)
    wi, wf, wl, wn, ws = (torch.as_tensor(v) for v in want)
    assert torch.equal(ids, wi) and torch.equal(frames, wf) and int(n) == int(wn), (got, want)
    for p, q in ((logp, wl), (score.reshape(1), ws.reshape(1))):
        if bar == 0.0:
            assert torch.equal(p, q), (p, q)
        else:
            assert p.dtype == q.dtype and bool(((p - q).abs() <= bar * q.abs().clamp(min=1.0)).all()), (p, q, (p - q).abs().max())


def whole(dec, x):
    """One stream fed in one call to slot 0 -> (ids, frames, logp, length, score)."""
    dec.start([0])
    S = dec.S
    mel = torch.zeros(S, x.shape[0], x.shape[1], dtype=x.dtype, device=x.device)
    mel[0] = x
    ids, counts = dec.feed(mel, [x.shape[0]] + [0] * (S - 1), [True] * S)
    hi, hl, hs = dec.hypotheses()
    n = int(hl[0])
    assert ids[0, : int(counts[0])].tolist() == hi[0, :n].tolist()
    ti, tf, tl = dec.timed_hypotheses()
    assert ti[0, :n].tolist() == hi[0, :n].tolist() and (tf[0, n:] == -1).all()
    return hi[0, :n].cpu(), tf[0, :n].cpu(), tl[0, :n].cpu(), n, hs[0].cpu()


def chunked(dec, x, slot, chunks, other=None):
    """The stream through `chunks` (mel frames per feed, the last one final) in `slot`; the other slots get `other`'s frames all along."""
    S, F = dec.S, x.shape[1]
    dec.start(list(range(S)))
    Tc, pos, opos, emitted = dec.Tc, 0, 0, []
    for k, c in enumerate(chunks):
        mel = torch.zeros(S, Tc, F, dtype=x.dtype, device=x.device)
        frames, final = [0] * S, [False] * S
        mel[slot, :c] = x[pos: pos + c]
        frames[slot], final[slot] = c, k == len(chunks) - 1
        pos += c
        if other is not None:
            oc = min(2 * (1 + k % 2), other.shape[0] - opos) // 2 * 2
            for s in range(S):
                if s != slot:
                    mel[s, :oc] = other[opos: opos + oc]
                    frames[s] = oc
            opos += oc
        ids, counts = dec.feed(mel, frames, final)
        emitted += ids[slot, : int(counts[slot])].tolist()
    hi, hl, hs = dec.hypotheses()
    n = int(hl[slot])
    assert emitted == hi[slot, :n].tolist()
    ti, tf, tl = dec.timed_hypotheses()
    return hi[slot, :n].cpu(), tf[slot, :n].cpu(), tl[slot, :n].cpu(), n, hs[slot].cpu()


MEL_CHUNKINGS = [[26], [2] * 13, [4, 0, 6, 2, 14], [10, 16, 0], [6, 8, 11]]  # (mel frames: reduction factor 2; an odd final chunk)


def test_streaming_decoder_chunked_equals_one_shot_and_the_batch_decoder():
    """ids, frames and lengths: exactly.  Scores and log-probabilities: to 1e-12 in float64, the bar of this file -- on the torch
    route torch's GEMMs round by their row count (the frames of a chunk, the slots), so its floats are not bitwise chunking-
    invariant (largest difference seen: about 2e-15); the engine is, bit for bit (tests/test_tdt_stream_gpu.py)."""
    model, _ = small_tdt_stream_model()
    g = torch.Generator().manual_seed(11)
    F = model.encoder.input_norm.num_features
    x, other = torch.randn(26, F, generator=g).double(), torch.randn(40, F, generator=g).double()
    want = whole(tdt.StreamingTDTGreedyDecoder(model, DUR, 1, 26, max_symbols_per_frame=2), x)
    assert want[3] >= 3 and len(set(want[1].tolist())) >= 2
    for chunks in MEL_CHUNKINGS:
        xs = x[: sum(chunks)]
        ref = want if sum(chunks) == 26 else whole(tdt.StreamingTDTGreedyDecoder(model, DUR, 1, 26, max_symbols_per_frame=2), xs)
        dec = tdt.StreamingTDTGreedyDecoder(model, DUR, 3, 26, max_symbols_per_frame=2, check_every=3)
        got = chunked(dec, xs, 2, chunks, other)
        equal_results(got, ref, BAR)
    # ids and frames: those of tdt_greedy_search_batch of the stream alone
    with torch.no_grad():
        enc = model.encoder(x[None])
    hyps, lengths, _, fr, _ = tdt.tdt_greedy_search_batch(model.prediction, model.joint, enc, torch.tensor([enc.shape[1]]), DUR,
                                                          max_symbols_per_frame=2, token_times=True)
    n = int(lengths[0])
    assert hyps[0, :n].tolist() == want[0].tolist() and fr[0, :n].tolist() == want[1].tolist()


def test_streaming_decoder_budget_and_constructor_checks():
    model, _ = small_tdt_stream_model()
    x = torch.randn(26, model.encoder.input_norm.num_features, generator=torch.Generator().manual_seed(11)).double()
    full = whole(tdt.StreamingTDTGreedyDecoder(model, DUR, 1, 26, max_symbols_per_frame=2), x)
    cut = whole(tdt.StreamingTDTGreedyDecoder(model, DUR, 1, 26, max_length=2, max_symbols_per_frame=2), x)
    assert cut[3] == 2 and cut[0].tolist() == full[0][:2].tolist()
    with pytest.raises(ValueError, match="max_symbols_per_frame"):
        tdt.StreamingTDTGreedyDecoder(model, DUR, 1, 26, max_symbols_per_frame=0)
    with pytest.raises(ValueError, match="durations"):
        tdt.StreamingTDTGreedyDecoder(model, [0, 0, 1], 1, 26)


def test_transcriber_with_tdt_durations_chunked_audio_equals_one_call():
    model, hp = small_tdt_stream_model()
    sr = 16000
    audio = fc.signal(1.0, sr, seed=21)
    n = len(audio)
    kw = dict(tdt_durations=DUR, max_length=40, max_symbols_per_frame=2)

    def run(chunks, slots, slot):
        tr = StreamingTranscriber(model, hp, sr, slots, 3000 if len(chunks) > 1 else n, **kw)
        assert isinstance(tr.decoder, tdt.StreamingTDTGreedyDecoder) and tr.decoder.Tc == tr.front.max_rows
        feed = tr.decoder.feed  # (the front end's rows are float32, the model of this file float64)
        tr.decoder.feed = lambda rows, counts, final: feed(rows.double(), counts, final)
        tr.start(list(range(slots)))
        rng, pos = np.random.default_rng(5), 0
        for i, k in enumerate(chunks):
            ks = [int(rng.integers(0, 1501)) for _ in range(slots)]
            ks[slot] = k
            au = torch.tensor(rng.normal(size=(slots, max(ks))).astype(np.float32) * 0.2)
            au[slot, :k] = torch.tensor(audio[pos: pos + k])
            fin = [False] * slots
            fin[slot] = i + 1 == len(chunks)
            tr.feed(au, ks, fin)
            pos += k
        ids, lengths, scores = tr.hypotheses()
        ti, tf, tl = tr.decoder.timed_hypotheses()
        m = int(lengths[slot])
        with pytest.raises(RuntimeError):
            tr.nbest()
        return ids[slot, :m], tf[slot, :m], tl[slot, :m], lengths[slot], scores[slot]

    one = run([n], 1, 0)
    rag = run(fc.ragged_chunks(n, seed=13), 4, 2)
    assert int(one[3]) >= 2
    equal_results((one[0], one[1], one[2], one[3], one[4]), (rag[0], rag[1], rag[2], rag[3], rag[4]), BAR)  # (as for the decoder above)
    words, final = StreamingTranscriber(model, hp, sr, 1, n, **kw).words(0)  # (timed words need no flag: the TDT decoder keeps the times)
    assert words == [] and final == 0


def test_transcriber_refuses_tdt_durations_with_beam():
    model, hp = small_tdt_stream_model()
    with pytest.raises(ValueError, match="tdt_durations"):
        StreamingTranscriber(model, hp, 16000, 1, 3000, beam=4, tdt_durations=DUR)
    assert isinstance(StreamingTranscriber(small_model(3).eval(), small_model(3).hp, 16000, 1, 3000).decoder, decoding.StreamingGreedyDecoder)
