"""The Python layer of LM shallow fusion on an MI355X: decoding.beam_search_batch / beam_decode_batch, StreamingBeamDecoder and
StreamingTranscriber with lm= through the engine (joint.BeamJoint / BeamStreamJoint calling the LM steps of include/rnnt_lm.h),
against the same decoders' torch route on a float64 copy of the model.  Ids, lengths, emission frames and states exactly; scores
and log-probabilities within the bars of tests/test_beam_search_gpu.py (1e-4 max(1, |s|))."""
import copy

import numpy as np
import pytest
import torch

from rnnt_speech_recognition_amd import decoding
from rnnt_speech_recognition_amd.joint import BeamJoint
from rnnt_speech_recognition_amd.lm import NgramLM
from tests.test_greedy_batch_gpu import _decode_model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _lm(V=12, blank=0):
    """A trigram LM over the model's 12 symbols, estimated from random sequences over 6 of them; weight 0.5, 0.25 a token."""
    rng = np.random.default_rng(3)
    seqs = [[int(x) for x in rng.choice([1, 2, 3, 5, 8, 9], size=int(rng.integers(1, 9)))] for _ in range(80)]
    return NgramLM.estimate(seqs, 3, blank, V, scale=0.5, token_bonus=0.25)


def _setup(seed=18):
    model = _decode_model(12)
    ref = copy.deepcopy(model).cpu().double().eval()
    torch.manual_seed(seed)
    mel = torch.randn(6, 30, 8)
    spec_lengths = torch.tensor([30, 25, 30, 4, 17, 0])
    return model, ref, _lm(), mel, spec_lengths


def _close(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    fin = torch.isfinite(b)
    assert torch.equal(torch.isfinite(a), fin)
    print(f"  worst score error {float((a[fin] - b[fin]).abs().max()) if fin.any() else 0.0:.3e}")
    assert (torch.abs(a[fin] - b[fin]) <= 1e-4 * torch.clamp(b[fin].abs(), min=1.0)).all(), (a, b)


@pytest.mark.parametrize("prediction", ["torch", "engine"])
@pytest.mark.parametrize("timed", [False, True])
def test_beam_search_batch_engine_route_matches_the_torch_route(prediction, timed):
    model, ref, g, mel, spec_lengths = _setup()
    assert BeamJoint(model.joint, 4, lm=g).engine and not BeamJoint(ref.joint, 4, lm=g).engine
    with torch.no_grad():
        enc = model.encoder(mel.to(DEV))
        frames = decoding.reduced_lengths(spec_lengths, model.hp.time_reduction_factor)
        got = decoding.beam_search_batch(model, enc, frames.to(DEV), beam=4, prediction=prediction, token_times=timed, lm=g)
        want = decoding.beam_search_batch(ref, enc.cpu().double(), frames, beam=4, token_times=timed, lm=g)
        plain = decoding.beam_search_batch(model, enc, frames.to(DEV), beam=4, prediction=prediction)
        best = decoding.beam_decode_batch(model, mel.to(DEV), spec_lengths.to(DEV), beam=4, prediction=prediction, token_times=timed, lm=g)
    assert len(got) == (5 if timed else 3)
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])  # ids, lengths: finalised order
    _close(got[2], want[2])
    assert (got[2][:, 1:] <= got[2][:, :-1]).all()  # re-sorted by the finalised score
    if timed:
        assert torch.equal(got[3].cpu(), want[3])  # the emission frames follow their hypotheses
        _close(got[4], want[4])
    assert not torch.equal(got[0], plain[0]), "the LM changes nothing: the case shows nothing"
    for x, y in zip(best, got):
        assert torch.equal(x, y[:, 0])


def test_streaming_beam_decoder_engine_route_matches_the_torch_route():
    model, ref, g, mel, _ = _setup(19)
    f = model.encoder.reduce.factor
    S, K, chunk = 3, 4, 4 * f
    dec = decoding.StreamingBeamDecoder(model, S, chunk, beam=K, max_length=24, lm=g)
    cpu = decoding.StreamingBeamDecoder(ref, S, chunk, beam=K, max_length=24, lm=g)
    assert dec.bj.engine and not cpu.bj.engine
    dec.start([0, 1, 2])
    cpu.start([0, 1, 2])
    x = mel[:S, :24]
    moved = 0
    for c in range(0, 24, chunk):
        frames = [chunk, chunk if c < 16 else 0, chunk]
        final = [c + chunk == 24, c + chunk == 16, c + chunk == 24]
        a = dec.feed(x[:, c: c + chunk].to(DEV), frames, final)
        b = cpu.feed(x[:, c: c + chunk].double(), frames, final)
        for p, q in zip(a, b):
            assert torch.equal(p.cpu(), q), c
        sa, sb = dec.lm_states().cpu(), cpu.lm_states()
        assert sa.shape == (S, K) and torch.equal(sa, sb), c
        moved += int((sa > 1).sum())
        for p, q in zip(dec.nbest()[:2], cpu.nbest()[:2]):
            assert torch.equal(p.cpu(), q), c
        _close(dec.nbest()[2], cpu.nbest()[2])
    assert moved > 0, "no hypothesis ever reached a state beyond <s> and the empty history: the case shows nothing"
    final = g.finalize(dec.nbest()[2], dec.lm_states())
    assert final.shape == (S, K) and (final <= dec.nbest()[2]).all()  # (log P(</s> | .) <= 0, the weight positive)


def test_streaming_transcriber_passes_the_lm_through():
    from rnnt_speech_recognition_amd.biasing import ContextGraph

    model = _decode_model(12)
    g = _lm()
    tr = decoding.StreamingTranscriber(model, model.hp, 16000, 2, 3000, beam=3, lm=g)
    assert tr.decoder.bj.lm is g and tr.decoder.bj.engine and tr.decoder.lm_states().shape == (2, 3)
    with pytest.raises(ValueError):
        decoding.StreamingTranscriber(model, model.hp, 16000, 2, 3000, lm=g)  # greedy: no LM
    with pytest.raises(ValueError):
        decoding.StreamingTranscriber(model, model.hp, 16000, 2, 3000, beam=3, lm=g, context=ContextGraph([(1, 2)], blank=0, vocab_size=12))
    tr.start([0, 1])
    torch.manual_seed(4)
    audio = torch.randn(2, 3000, device=DEV) * 0.1
    tr.feed(audio, [3000, 3000], [True, True])
    ids, lengths, scores = (x.cpu() for x in tr.decoder.nbest())
    states = tr.decoder.lm_states().cpu()
    for s in range(2):  # every live hypothesis sits in the state its tokens lead to from the sentence start
        for k in range(3):
            if torch.isfinite(scores[s, k]):
                assert g.walk(ids[s, k, : int(lengths[s, k])].tolist())[0] == int(states[s, k]), (s, k)
