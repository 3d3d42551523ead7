"""Streaming beam search with several symbols per frame on CPU tensors: joint.MultiBeamStreamJoint's torch mirror,
decoding.StreamingMultiBeamDecoder and StreamingTranscriber(beam=, symbols_per_frame=) against the float64 restatement of
include/rnnt_beam_multi.h run over each stream's whole utterance with the frame rows of include/rnnt_beam_multi_stream.h
(tests/multibeam_stream_cases.py).  Ids, lengths, frames, parents, emitted and both stable lengths exactly; float64 scores to
1e-12 max(1, |s|): both sides add at most a few hundred float64 terms to a score, each rounded to 2^-53 of it."""
import math

import numpy as np
import pytest
import torch

from rnnt_speech_recognition_amd import decoding
from rnnt_speech_recognition_amd import joint as jmod
from tests import multibeam_stream_cases as sc_
from tests.test_frontend import small_model
from tests.test_multibeam import MirrorMulti, _joint_module


def exact_fn(sc):
    """The logits the mirror forms from the scripted rows, in float64: c tanh of the float32 pred_proj row."""
    sj = sc.joint
    return lambda key, t, y: sj.c * np.tanh(sj.pred_rows(sc.script(key, t, y))[0, : sj.V].astype(np.float64))


SCENARIOS = sc_.cpu_scenarios(exact_fn)


class MirrorStream:
    def __init__(self, sc, timed=True):
        self.sc = sc
        jl = _joint_module(sc.joint, sc.blank)
        with torch.no_grad():  # W1 [H, J] = 0, b1 = 0: enc_proj is b1 whatever the frames hold
            jl.W1 = torch.nn.Parameter(torch.zeros(sc_.H, sc.joint.J, dtype=torch.float64))
            jl.b1.zero_()
        self.mj = jmod.MultiBeamStreamJoint(jl, beam=sc.K, symbols_per_frame=sc.E, token_times=timed)
        self.timed = timed

    def begin(self):
        self.mj.begin(self.sc.S, self.sc.Tc, self.sc.N)
        assert not self.mj.engine

    def feed(self, enc, fr, rs, fi):
        self.mj.feed(None if enc is None else torch.tensor(enc, dtype=torch.float64), fr, rs, fi)

    def step(self, rows):
        with torch.no_grad():
            p, e = self.mj.step(pred_proj=torch.tensor(rows, dtype=torch.float64))
        return p.numpy(), e.numpy()

    def results(self):
        r = tuple(x.numpy() for x in self.mj.results())
        return r if self.timed else r + (None, None)


def _score_ok(got, want, rounds, ref):
    return abs(got - want) <= 1e-12 * max(1.0, abs(want))


def _run(sc, timed=True, every_step=True):
    out = sc_.run_streams(MirrorStream(sc, timed), sc, exact_fn(sc), _score_ok, compare_every_step=every_step)
    sc_.check_expectations(sc, out)
    return out


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_scenarios_on_the_torch_mirror(name):
    sc = SCENARIOS[name]
    out = _run(sc)
    print(sc_.describe(sc, out))
    for n, st in enumerate(sc.streams):
        assert out.results[n] is not None, (n, "the stream never owned its slot")


def test_the_scenario_list_covers_what_the_contract_names():
    names = list(SCENARIOS)
    for chunking in sc_.CHUNKINGS:
        assert any(n.startswith(f"chunks-{chunking}-") for n in names)
    for part in ("frame-merge", "overflow-boundary", "slots-0of4", "slots-3of4", "final", "capacity-N3", "capacity-N1", "empty-turn",
                 "nan-rows", "ties"):
        assert any(n.startswith(part) for n in names), part
    assert {sc.E for sc in SCENARIOS.values()} >= {1, 2, 3, 8} and {sc.K for sc in SCENARIOS.values()} >= {1, 4, 16}
    assert any(sc.Tc == 1 for sc in SCENARIOS.values())
    for sc in SCENARIOS.values():
        assert sc.S * 2 * sc.K <= 1024
        for st in sc.streams:
            assert max(st.chunks + st.after) <= sc.Tc and sum(st.chunks) == st.T


def test_frozen_slots_and_frame_merges_are_seen():
    out = _run(SCENARIOS[sc_.slots_scenario(2).name], every_step=False)
    assert out.frozen_steps >= 10  # slots whose chunk is shorter than the feed's longest freeze mid-feed
    out = _run(SCENARIOS[sc_.frame_merge_scenario().name], every_step=False)
    assert sum(t.frame_merges_reported for t in out.refs) >= 1


@pytest.mark.parametrize("name", [n for n in sc_.CHUNKINGS if n != "one"])
def test_every_chunking_gives_the_bits_of_one_chunk(name):
    one = _run(sc_.chunking_scenario("one"), every_step=False).results[0]
    got = _run(sc_.chunking_scenario(name), every_step=False).results[0]
    assert sc_.same_bits(one, got)
    untimed = _run(sc_.chunking_scenario(name), timed=False, every_step=False).results[0]
    assert sc_.same_bits(one[:4], untimed[:4]) and untimed[4] is None


@pytest.mark.parametrize("slot", range(4))
def test_every_slot_gives_the_bits_of_the_one_slot_decoder(slot):
    one = _run(sc_.chunking_scenario("one"), every_step=False).results[0]
    assert sc_.same_bits(one, _run(sc_.slots_scenario(slot), every_step=False).results[0])


@pytest.mark.parametrize("K,E,dtype", [(4, 2, 0), (3, 3, 1), (16, 1, 0)])
def test_the_stream_mirror_equals_the_offline_mirror(K, E, dtype):
    """The mirror's stream against the mirror's offline MultiBeamJoint on the same frames: same bits."""
    sc = sc_.chunking_scenario("cuts", K=K, E=E, dtype=dtype)
    got = _run(sc, every_step=False).results[0]
    sj, T, N = sc.joint, sc_.T13, sc.N
    eng = MirrorMulti(sj, 1, K, E, N, T, [T], sc.blank)
    eng.begin()
    seqs = [()] * (2 * K)
    for step in range(T * (E + 1)):
        rows = np.stack([sj.pred_rows(sc.script(0, step // (E + 1), y))[0] for y in seqs])
        p, e = eng.step(rows)
        seqs = [seqs[q] + ((v,) if v >= 0 else ()) for q, v in zip(p.tolist(), e.tolist())]
    hyps, lengths, scores = eng.results()
    assert sc_.same_bits((hyps[0], lengths[0], scores[0]), got[:3])


# ---- the decoder and the transcriber on a small Transducer --------------------------------------------
def _offline(model, mel, E, K=3, max_length=None):
    with torch.no_grad():
        enc = model.encoder(mel)
    frames = torch.tensor([enc.shape[1]] * mel.shape[0])
    return decoding.beam_search_batch(model, enc, frames, beam=K, symbols_per_frame=E, max_length=max_length)


@pytest.mark.parametrize("E", [1, 2])
def test_streaming_decoder_follows_the_offline_search_and_its_own_one_chunk_run(E):
    torch.manual_seed(3)
    model = small_model().eval()
    f = int(model.encoder.reduce.factor)
    F = int(model.encoder.input_norm.num_features)
    T = 6 * f
    mel = torch.randn(2, T, F)
    N = (T // f) * E
    ids0, len0, sc0 = _offline(model, mel, E, max_length=N)

    def run(chunks, slots, slot):
        dec = decoding.StreamingMultiBeamDecoder(model, slots, T, beam=3, symbols_per_frame=E, max_length=N, token_times=True)
        dec.start([slot])
        at = 0
        for i, n in enumerate(chunks):
            chunk = torch.zeros(slots, T, F)
            chunk[slot, :n] = mel[0, at: at + n]
            fr = [0] * slots
            fr[slot] = n
            best = dec.feed(chunk, fr, [i + 1 == len(chunks)] * slots)
            at += n
        return dec, best

    dec, best = run([T], 1, 0)
    ids, lengths, scores = dec.nbest()
    assert ids.shape == (1, 3, N) and torch.equal(ids[0], ids0[0]) and torch.equal(lengths[0], len0[0])
    fin = torch.isfinite(sc0[0])
    assert torch.allclose(scores[0][fin].double(), sc0[0][fin].double(), rtol=1e-5, atol=1e-5)
    assert torch.equal(best[0][0], ids[0, 0]) and int(best[1][0]) == int(lengths[0, 0]) and 0 <= int(best[2][0]) <= int(lengths[0, 0])
    tids, tfr = dec.timed_hypotheses()
    n = int(lengths[0, 0])
    assert torch.equal(tids[0], ids[0, 0]) and (tfr[0, n:] == -1).all()
    fr = tfr[0, :n].tolist()
    assert fr == sorted(fr) and all(0 <= x < T // f for x in fr) and all(fr.count(x) <= E for x in set(fr))
    assert len(dec.timed_nbest()) == 4 and int(dec.timed_stable_lengths()[0]) <= int(best[2][0])
    dec2, _ = run([2 * f, f, 3 * f], 3, 2)
    for a, b in zip(dec.timed_nbest(), dec2.timed_nbest()):
        assert torch.equal(a[0], b[2])
    assert torch.equal(dec.timed_stable_lengths()[0], dec2.timed_stable_lengths()[2])
    assert int(dec2.nbest()[1][0].sum()) == 0 and (dec2.nbest()[2][0] == -math.inf).all()  # a never-started slot


def test_value_errors():
    model = small_model().eval()
    D = decoding.StreamingMultiBeamDecoder
    for kw in (dict(beam=0), dict(beam=17), dict(symbols_per_frame=0), dict(symbols_per_frame=9), dict(max_length=0),
               dict(context=object()), dict(lm=object())):
        with pytest.raises(ValueError):
            D(model, 2, 8, **kw)
    with pytest.raises(ValueError):
        D(model, 129, 8, beam=4)  # 129 * 2 * 4 rows
    dec = D(model, 1, 8)
    with pytest.raises(RuntimeError):
        dec.timed_hypotheses()
    mj = jmod.MultiBeamStreamJoint(model.joint, 4, 2)
    for args in ((0, 4, 4), (129, 4, 4), (1, 0, 4), (1, 4, 0)):
        with pytest.raises(ValueError):
            mj.begin(*args)
    mj.begin(1, 4, 4)
    with pytest.raises(ValueError):
        mj.feed(torch.zeros(1, 5, mj.joint.W1.shape[0]), [5])
    with pytest.raises(ValueError):
        jmod.MultiBeamStreamJoint(model.joint, 4, 9)


def test_transcriber_selects_the_decoder_and_refuses_what_does_not_go_with_it():
    torch.manual_seed(5)
    model = small_model().eval()
    hp = model.hp
    sr = 16000
    T = decoding.StreamingTranscriber
    tr = T(model, hp, sr, 2, 4000, beam=3, symbols_per_frame=2, token_times=True)
    assert type(tr.decoder) is decoding.StreamingMultiBeamDecoder and tr.decoder.E == 2 and tr.decoder.K == 3
    assert type(T(model, hp, sr, 2, 4000, beam=3).decoder) is decoding.StreamingBeamDecoder  # without it: what it was
    for kw in (dict(symbols_per_frame=2), dict(beam=3, symbols_per_frame=2, context=object()), dict(beam=3, symbols_per_frame=2, lm=object()),
               dict(symbols_per_frame=2, tdt_durations=[0, 1]), dict(symbols_per_frame=2, tdt_durations=[0, 1], tdt_beam=2)):
        with pytest.raises(ValueError):
            T(model, hp, sr, 2, 4000, **kw)
    tr.start([0, 1])
    audio = 0.1 * torch.randn(2, 4000)
    best = tr.feed(audio, [4000, 2500], [False, True])
    assert len(best) == 3 and best[0].shape[0] == 2
    ids, lengths, scores = tr.nbest()
    assert ids.shape[:2] == (2, 3) and torch.equal(tr.hypotheses()[0], ids[:, 0])
    with pytest.raises(RuntimeError, match="log-probabilities"):
        tr.words(0)
    with pytest.raises(ValueError):  # the offline search keeps no token times
        with torch.no_grad():
            enc = model.encoder(torch.randn(1, 4 * int(model.encoder.reduce.factor), int(model.encoder.input_norm.num_features)))
        decoding.beam_search_batch(model, enc, torch.tensor([enc.shape[1]]), beam=2, symbols_per_frame=2, token_times=True)
