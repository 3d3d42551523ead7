"""Streaming TDT beam search on the torch route (tdt.TDTBeamStreamJoint / tdt.StreamingTDTBeamDecoder on CPU tensors): every scenario
of tests/tdt_beam_stream_cases.py against the float64 restatement of each stream's whole utterance at every step -- ids, lengths,
cursors, frames, durations, both stable lengths, parents and emitted exactly, scores to 1e-12 (float64 on both sides) --, the
chunking equivalence bit for bit, the capacity rule, beam = 1 against StreamingTDTGreedyDecoder, and the transcriber's refusals."""
import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import tdt
from rnnt_speech_recognition_amd.decoding import StreamingTranscriber
from tests import frontend_cases as fc
from tests import tdt_beam_stream_cases as sc_
from tests.test_tdt_greedy import cpu_logits
from tests.test_tdt_stream import DUR, small_tdt_stream_model


class CpuStreamJoint:
    """W1 = 0, b1 = 0 in float64: enc_proj is exactly 0 and, with pred_proj = the case's row, the logits are tanh(row) @ W2 + b2."""

    def __init__(self, case):
        self.W1 = torch.zeros(sc_.H, case.J, dtype=torch.float64)
        self.b1 = torch.zeros(case.J, dtype=torch.float64)
        self.W2 = torch.from_numpy(case.W2).double()
        self.b2 = torch.from_numpy(case.b2).double()
        self.blank_label = case.blank


class TorchEngine:
    def __init__(self, sc, token_times=True, diag=True):
        self.sc, self.diag, self.tops = sc, diag, None
        self.jb = tdt.TDTBeamStreamJoint(CpuStreamJoint(sc.case), sc.case.durations, sc.K, token_times=token_times)
        assert not self.jb.engine

    def begin(self):
        self.jb.begin(self.sc.S, self.sc.Tc, self.sc.N)

    def feed(self, enc, frames, reset, final):
        self.jb.feed(None if enc is None else torch.from_numpy(enc).double(), frames, reset, final)

    def step(self, rows):
        R = rows.shape[0]
        tops = torch.full((R, self.sc.K), -7, dtype=torch.int32) if self.diag else None
        parents, emitted = self.jb.step(pred_proj=torch.from_numpy(rows).double(), topk_symbols=tops)
        self.tops = None if tops is None else tops.numpy()
        return parents.numpy(), emitted.numpy()

    def results(self):
        out = tuple(x.numpy() for x in self.jb.results())
        return out if len(out) == 8 else out + (None, None, None)


def close(got, want, steps, ref):
    return abs(got - want) <= 1e-12


def _run(sc, **kw):
    return sc_.run_streams(TorchEngine(sc, **kw), sc, cpu_logits(sc.case), close)


def test_exports_and_arguments():
    assert pkg.TDTBeamStreamJoint is tdt.TDTBeamStreamJoint and pkg.StreamingTDTBeamDecoder is tdt.StreamingTDTBeamDecoder
    assert issubclass(tdt.TDTBeamStreamJoint, tdt.TDTBeamJoint) and issubclass(tdt.StreamingTDTBeamDecoder, pkg.StreamingBeamDecoder)
    joint = CpuStreamJoint(sc_.chunking_scenario("one").case)
    with pytest.raises(ValueError):
        tdt.TDTBeamStreamJoint(joint, sc_.D5, 17)
    with pytest.raises(ValueError):
        tdt.TDTBeamStreamJoint(joint, [0, 0, 1], 4)
    jb = tdt.TDTBeamStreamJoint(joint, sc_.D5, 16)
    with pytest.raises(ValueError):
        jb.begin(65, 4, 8)  # slots * beam > 1024
    with pytest.raises(ValueError):
        jb.begin(2, 4, 0)
    jb.begin(2, 4, 8)
    with pytest.raises(ValueError):
        jb.feed(torch.zeros(2, 5, sc_.H, dtype=torch.float64), [5, 5])
    hyps, lengths, scores, stable, cursors = jb.results()  # never started: empty beams
    assert hyps.shape == (2, 16, 8) and not hyps.any() and not lengths.any() and (scores == -np.inf).all()
    assert (cursors == -1).all() and not stable.any()


@pytest.mark.parametrize("name", list(sc_.CHUNKINGS))
@pytest.mark.parametrize("dtype", [0, 1])
def test_every_chunking_matches_the_restatement_and_the_single_chunk(name, dtype):
    one = _run(sc_.chunking_scenario("one", dtype=dtype))
    out = _run(sc_.chunking_scenario(name, dtype=dtype))
    assert sc_.same_bits(out.results[0], one.results[0])
    ev = out.refs[0].ev
    assert ev.merges >= 1 and ev.worst_gap_ratio > 3.0 and out.steps == 13 and out.tops_checked == ev.active_rows
    assert out.results[0][2].dtype == np.float64 and out.results[0][0].shape == (4, 13)


@pytest.mark.parametrize("chunk", [14, 1, 2, 3])
def test_a_carry_that_outlives_several_feeds(chunk):
    one = _run(sc_.long_carry_scenario(14))
    out = _run(sc_.long_carry_scenario(chunk))
    assert sc_.same_bits(out.results[0], one.results[0])
    ev = out.refs[0].ev
    assert ev.idle_full >= 4 and ev.past_end >= 1 and 8 in ev.durations_used


@pytest.mark.parametrize("K", [2, 4])
def test_merges_and_non_merges_across_a_boundary(K):
    """With 1-frame chunks every merge of a stay with an expansion, and every pair kept apart, spans a feed."""
    one = _run(sc_.boundary_merge_scenario(9, K))
    for chunk in (1, 2):
        out = _run(sc_.boundary_merge_scenario(chunk, K))
        assert sc_.same_bits(out.results[0], one.results[0])
        ev = out.refs[0].ev
        assert ev.stay_merges >= 1 and ev.kept_apart >= 1 and ev.aligned_later >= 1


@pytest.mark.parametrize("slot", [0, 2, 3])
def test_the_same_stream_in_any_slot_beside_other_traffic(slot):
    one = _run(sc_.chunking_scenario("one"))
    out = _run(sc_.slots_scenario(slot))
    assert sc_.same_bits(out.results[0], one.results[0])
    assert out.frozen_steps > 0
    assert sc_.same_bits(out.results[3], _run(sc_.slots_scenario(0)).results[3])  # the restarted slot's stream too


def test_final_chunk_freezes_the_slot_until_a_reset():
    out = _run(sc_.final_scenario())
    one = _run(sc_.chunking_scenario("one"))
    assert sc_.same_bits(out.results[1], one.results[0])  # the slot reused by a reset: the whole utterance
    cut = out.results[0]
    assert out.refs[0].t == 9 and (cut[4][cut[1] > 0] >= 9).all()  # every cursor at or beyond the final chunk's end
    assert out.refs[0].ev.past_end >= 1 and out.frozen_steps > 0


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("chunks", [(10,), (2, 1, 3, 4), (1,) * 10])
def test_a_full_hypothesis_offers_its_blank_alone(N, chunks):
    sc = sc_.n_rule_scenario(N, chunks=chunks)
    out = _run(sc)
    ref = out.refs[0]
    assert ref.full_rows > 0 and ref.blank_outside > 0 and (N == 1 or ref.mixed_frames > 0)
    assert out.tops_checked > 0 and (out.results[0][1] <= N).all() and (out.results[0][1] == N).any()
    assert sc_.same_bits(out.results[0], _run(sc_.n_rule_scenario(N, chunks=(10,))).results[0])


def test_the_capacity_restatement_is_the_offline_one_where_it_cannot_fire():
    sc = sc_.chunking_scenario("one")
    fn = cpu_logits(sc.case)
    a = sc_.make_ref(sc, sc.streams[0], fn)
    sc.n_rule = True
    b = sc_.make_ref(sc, sc.streams[0], fn)
    for _ in range(13):
        assert a.step() == b.step() and a.beams == b.beams
    assert b.full_rows == 0


def test_a_row_of_nan_logits_carries_the_beam_over():
    out = _run(sc_.nan_scenario())
    assert out.refs[0].ev.carried == [(0, 4)] and out.refs[0].ev.dropped >= 1


def test_untimed_gives_the_same_ids_and_scores():
    sc = sc_.chunking_scenario("cuts")
    a, b = _run(sc), _run(sc, token_times=False)
    assert sc_.same_bits(a.results[0][:5], b.results[0][:5]) and b.results[0][5] is None


def _same(a, b):
    """Two results tuples of one stream: integer tensors exactly, scores to 1e-12 (on the torch route torch's GEMMs round by their
    row count, so its floats are not bitwise chunking-invariant: tests/test_tdt_stream.py; the engine is, bit for bit)."""
    for x, y in zip(a, b):
        if x.dtype.is_floating_point:
            assert bool(((x - y).abs() <= 1e-12 * y.abs().clamp(min=1.0))[torch.isfinite(y)].all()) and torch.equal(torch.isfinite(x), torch.isfinite(y))
        else:
            assert torch.equal(x, y), (x, y)


def _feed_all(dec, x, slot, chunks):
    dec.start([slot])
    at = 0
    for i, n in enumerate(chunks):
        mel = torch.zeros(dec.S, 26, x.shape[1], dtype=x.dtype)
        mel[slot, :n] = x[at:at + n]
        fr, fi = [0] * dec.S, [False] * dec.S
        fr[slot], fi[slot] = n, i + 1 == len(chunks)
        dec.feed(mel, fr, fi)
        at += n
    return dec


def test_decoder_chunkings_and_beam_1_is_greedy():
    model, _ = small_tdt_stream_model()
    x = torch.randn(26, model.encoder.input_norm.num_features, generator=torch.Generator().manual_seed(11)).double()
    res = lambda d, s: tuple(v[s] for v in d.timed_nbest() + (d.timed_stable_lengths(), d.cursors()))  # noqa: E731
    want = _feed_all(tdt.StreamingTDTBeamDecoder(model, DUR, 1, 26, beam=3, token_times=True), x, 0, [26])
    assert int(want.hypotheses()[1][0]) >= 2
    for chunks in ([2] * 13, [4, 0, 6, 2, 14], [10, 16, 0]):
        got = _feed_all(tdt.StreamingTDTBeamDecoder(model, DUR, 3, 26, beam=3, token_times=True), x, 2, chunks)
        _same(res(got, 2), res(want, 0))
    ids, fr, du = got.timed_hypotheses()
    assert torch.equal(ids[2], got.timed_nbest()[0][2, 0]) and torch.equal(fr[2], got.timed_nbest()[3][2, 0])
    ids2, lengths, stable = got.feed(torch.zeros(3, 2, x.shape[1]).double(), [0, 0, 0], [False] * 3)  # (a finished slot: nothing moves)
    assert torch.equal(ids2[2], ids[2]) and bool((got.timed_stable_lengths() <= stable).all()) and bool((stable <= lengths).all())
    # beam = 1: the greedy decoder with one symbol per frame, ids and frames
    b1 = _feed_all(tdt.StreamingTDTBeamDecoder(model, DUR, 1, 26, beam=1, token_times=True), x, 0, [6, 20])
    gr = _feed_all(tdt.StreamingTDTGreedyDecoder(model, DUR, 1, 26, max_symbols_per_frame=1, max_length=64), x, 0, [6, 20])
    ids, fr, _ = b1.timed_hypotheses()
    gi, gf, _ = gr.timed_hypotheses()
    n = int(b1.hypotheses()[1][0])
    assert n >= 2 and n == int(gr.hypotheses()[1][0]) and ids[0, :n].tolist() == gi[0, :n].tolist() and fr[0, :n].tolist() == gf[0, :n].tolist()
    with pytest.raises(RuntimeError):
        tdt.StreamingTDTBeamDecoder(model, DUR, 1, 26).timed_nbest()
    with pytest.raises(TypeError):
        tdt.StreamingTDTBeamDecoder(model, DUR, 1, 26, context=object())
    with pytest.raises(ValueError, match="durations"):
        tdt.StreamingTDTBeamDecoder(model, [0, 0, 1], 1, 26)


def test_transcriber_takes_tdt_beam_and_refuses_the_rest():
    model, hp = small_tdt_stream_model()
    sr = 16000
    with pytest.raises(ValueError, match="tdt_beam="):
        StreamingTranscriber(model, hp, sr, 1, 3000, beam=4, tdt_durations=DUR)
    with pytest.raises(ValueError, match="tdt_durations"):
        StreamingTranscriber(model, hp, sr, 1, 3000, tdt_beam=4)
    with pytest.raises(ValueError):
        StreamingTranscriber(model, hp, sr, 1, 3000, tdt_durations=DUR, tdt_beam=4, lm=object())
    audio = fc.signal(1.0, sr, seed=21)
    n = len(audio)
    kw = dict(tdt_durations=DUR, tdt_beam=3, max_length=40, token_times=True)

    def run(chunks, slots, slot):
        tr = StreamingTranscriber(model, hp, sr, slots, 3000 if len(chunks) > 1 else n, **kw)
        assert isinstance(tr.decoder, tdt.StreamingTDTBeamDecoder) and tr.decoder.K == 3 and tr.decoder.Tc == tr.front.max_rows
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
        assert torch.equal(tr.nbest()[0], tr.decoder.timed_nbest()[0])
        with pytest.raises(RuntimeError, match="log-probabilities"):
            tr.words(slot)
        return tuple(v[slot] for v in tr.decoder.timed_nbest() + (tr.decoder.timed_stable_lengths(), tr.decoder.cursors()))

    one = run([n], 1, 0)
    assert int(one[1][0]) >= 2
    _same(run(fc.ragged_chunks(n, seed=13), 4, 2), one)
