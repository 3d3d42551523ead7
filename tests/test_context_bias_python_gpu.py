"""The Python layer of contextual biasing on an MI355X: decoding.beam_search_batch / beam_decode_batch and StreamingBeamDecoder
with context= through the engine (joint.BeamJoint / BeamStreamJoint calling the biased steps of include/rnnt_bias.h), against
the same decoders' torch route on a float64 copy of the model.  Ids, lengths, emission frames and states exactly; scores and
log-probabilities within the bars of tests/test_beam_search_gpu.py (1e-4 max(1, |s|))."""
import copy

import numpy as np
import pytest
import torch

from rnnt_speech_recognition_amd import decoding
from rnnt_speech_recognition_amd.biasing import ContextGraph
from rnnt_speech_recognition_amd.joint import BeamJoint
from tests import bias_cases as bc
from tests.test_greedy_batch_gpu import _decode_model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _setup(seed=18):
    model = _decode_model(12)
    ref = copy.deepcopy(model).cpu().double().eval()
    phrases, boosts = bc.random_phrases(np.random.default_rng(3), 12, 0, 10, max_len=3)
    g = ContextGraph(phrases, boost=boosts, blank=0, vocab_size=12)
    torch.manual_seed(seed)
    mel = torch.randn(6, 30, 8)
    spec_lengths = torch.tensor([30, 25, 30, 4, 17, 0])
    return model, ref, g, mel, spec_lengths


def _close(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    fin = torch.isfinite(b)
    assert torch.equal(torch.isfinite(a), fin)
    assert (torch.abs(a[fin] - b[fin]) <= 1e-4 * torch.clamp(b[fin].abs(), min=1.0)).all(), (a, b)


@pytest.mark.parametrize("prediction", ["torch", "engine"])
@pytest.mark.parametrize("timed", [False, True])
def test_beam_search_batch_engine_route_matches_the_torch_route(prediction, timed):
    model, ref, g, mel, spec_lengths = _setup()
    assert BeamJoint(model.joint, 4, context=g).engine and not BeamJoint(ref.joint, 4, context=g).engine
    with torch.no_grad():
        enc = model.encoder(mel.to(DEV))
        frames = decoding.reduced_lengths(spec_lengths, model.hp.time_reduction_factor)
        got = decoding.beam_search_batch(model, enc, frames.to(DEV), beam=4, prediction=prediction, token_times=timed, context=g)
        want = decoding.beam_search_batch(ref, enc.cpu().double(), frames, beam=4, token_times=timed, context=g)
        plain = decoding.beam_search_batch(model, enc, frames.to(DEV), beam=4, prediction=prediction)
        best = decoding.beam_decode_batch(model, mel.to(DEV), spec_lengths.to(DEV), beam=4, prediction=prediction, token_times=timed,
                                          context=g)
    assert len(got) == (5 if timed else 3)
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])  # ids, lengths: finalised order
    _close(got[2], want[2])
    assert (got[2][:, 1:] <= got[2][:, :-1]).all()  # re-sorted by the finalised score
    if timed:
        assert torch.equal(got[3].cpu(), want[3])  # the emission frames follow their hypotheses
        _close(got[4], want[4])
    assert not torch.equal(got[0], plain[0]), "the context changes nothing: the case shows nothing"
    for x, y in zip(best, got):
        assert torch.equal(x, y[:, 0])


def test_streaming_beam_decoder_engine_route_matches_the_torch_route():
    model, ref, g, mel, _ = _setup(19)
    f = model.encoder.reduce.factor
    S, K, chunk = 3, 4, 4 * f
    dec = decoding.StreamingBeamDecoder(model, S, chunk, beam=K, max_length=24, context=g)
    cpu = decoding.StreamingBeamDecoder(ref, S, chunk, beam=K, max_length=24, context=g)
    assert dec.bj.engine and not cpu.bj.engine
    dec.start([0, 1, 2])
    cpu.start([0, 1, 2])
    x = mel[:S, :24]
    off_root = 0
    for c in range(0, 24, chunk):
        frames = [chunk, chunk if c < 16 else 0, chunk]
        final = [c + chunk == 24, c + chunk == 16, c + chunk == 24]
        a = dec.feed(x[:, c: c + chunk].to(DEV), frames, final)
        b = cpu.feed(x[:, c: c + chunk].double(), frames, final)
        for p, q in zip(a, b):
            assert torch.equal(p.cpu(), q), c
        sa, sb = dec.bias_states().cpu(), cpu.bias_states()
        assert sa.shape == (S, K) and torch.equal(sa, sb), c
        off_root += int((sa != 0).sum())
        for p, q in zip(dec.nbest()[:2], cpu.nbest()[:2]):
            assert torch.equal(p.cpu(), q), c
        _close(dec.nbest()[2], cpu.nbest()[2])
    assert off_root > 0, "no hypothesis ever left the root: the case shows nothing"
    final = g.finalize(dec.nbest()[2], dec.bias_states())
    assert final.shape == (S, K) and (final <= dec.nbest()[2]).all()
