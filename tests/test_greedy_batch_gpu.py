"""Batched greedy decoding on an MI355X: the step kernel against compute_rnnt_joint_logits per hypothesis (bitwise argmax and
max logit), the whole decoder against a float64 restatement of utils/decoding.py, no host sync per step, robustness."""

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib, decoding, joint as jmod
from tests.test_frontend import _joint_forward_f16, small_model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _opts(blank, T):
    return _lib.make_options(torch.cuda.current_stream().cuda_stream, blank, T, 1)


def _ref_logits(ep, pp, W2, b2, dtype):
    """compute_rnnt_joint_logits for ONE hypothesis (minibatch = maxT = maxU = 1); the vocabulary padded as joint_logits pads it."""
    J, V = W2.shape
    Vp = V if dtype == 0 else max(128, (V + 127) // 128 * 128)
    if Vp != V:
        W2 = torch.nn.functional.pad(W2, (0, Vp - V)).contiguous()
        b2 = torch.nn.functional.pad(b2, (0, Vp - V), value=-1.0e4).contiguous()
    ws = torch.empty(_lib.joint_workspace_bytes(1, 1, 1, J, Vp), dtype=torch.uint8, device=DEV)
    out = torch.empty(1, 1, 1, Vp, dtype=torch.float32, device=DEV)
    o = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, 1, 1)
    _lib.check(_lib.load().compute_rnnt_joint_logits(ep.data_ptr(), pp.data_ptr(), W2.data_ptr(), b2.data_ptr(), J, Vp, 1,
                                                     out.data_ptr(), dtype, ws.data_ptr(), o), "compute_rnnt_joint_logits")
    return out[0, 0, 0]


STEP_CASES = ([(0, J, V) for V in (12, 28, 64, 128) for J in (64, 640)] + [(0, 704, 28)]
              + [(1, J, V) for V in (128, 1024, 4096, 8192) for J in (128, 640)] + [(1, 256, 1000)])


@pytest.mark.parametrize("case", range(len(STEP_CASES)))
def test_step_matches_the_logits_entry_per_hypothesis(case):
    dtype, J, V = STEP_CASES[case]
    B = (1, 33, 64, 200)[case % 4]
    T = 5
    g = torch.Generator().manual_seed(1000 + case)
    enc = torch.randn(B, T, J, generator=g)
    pred = torch.randn(B, J, generator=g)
    if B > 2:  # one enc row and one pred row beyond the e^{2x} table range: both tanh routes in one step
        enc[1, 0] *= 60.0
        pred[2] *= 60.0
    W2 = torch.rand(J, V, generator=g) * 2 - 1
    W2 *= (6.0 / (J + V)) ** 0.5 * (3.0 if dtype == 0 else 12.0)
    b2 = 0.1 * torch.randn(V, generator=g)
    if case == len(STEP_CASES) - 1:  # every real logit far below zero: a padding column that took part would win
        b2 -= 2.0e4
    enc, pred, W2, b2 = (x.to(DEV).contiguous() for x in (enc, pred, W2, b2))
    frames = torch.full((B,), T, dtype=torch.int32, device=DEV)
    ws = torch.empty(_lib.greedy_workspace_bytes(T, B, J, V, dtype), dtype=torch.uint8, device=DEV)
    hyps = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    lengths, emitted, done = (torch.zeros(n, dtype=torch.int32, device=DEV) for n in (B, B, 1))
    scores = torch.zeros(B, dtype=torch.float32, device=DEV)
    stats = torch.full((B, 2), float("nan"), dtype=torch.float32, device=DEV)
    lib = _lib.load()
    _lib.check(lib.compute_rnnt_greedy_begin(enc.data_ptr(), frames.data_ptr(), None, W2.data_ptr(), b2.data_ptr(), J, V, B, 0,
                                             dtype, ws.data_ptr(), _opts(0, T)), "begin")
    _lib.check(lib.compute_rnnt_greedy_step(pred.data_ptr(), hyps.data_ptr(), 4, lengths.data_ptr(), scores.data_ptr(),
                                            emitted.data_ptr(), done.data_ptr(), stats.data_ptr(), J, V, B, dtype, ws.data_ptr(),
                                            _opts(0, T)), "step")
    torch.cuda.synchronize()
    em, st = emitted.cpu(), stats.cpu()
    for b in range(B):
        ref = _ref_logits(enc[b, 0].contiguous(), pred[b].contiguous(), W2, b2, dtype)[:V].cpu()
        k = int(torch.argmax(ref))
        got_k = int(em[b]) if int(em[b]) >= 0 else 0
        assert got_k == k and got_k < V, (case, b, got_k, k)
        assert st[b, 0].item() == ref[k].item(), (case, b, st[b, 0].item(), ref[k].item())  # bitwise
        lse = float(torch.logsumexp(ref.double(), 0))
        assert abs(st[b, 1].item() - lse) <= 1e-6 * max(1.0, abs(lse)), (case, b, st[b, 1].item(), lse)
        assert abs(scores[b].item() - (ref[k].item() - lse)) <= 1e-5 * max(1.0, abs(lse))
    assert (lengths.cpu() == (em >= 0).int()).all()


def _decode_model(vocab):
    model = small_model(3) if vocab == 12 else small_model(3, vocab_size=vocab, joint_net_size=128, projection_size=32)
    with torch.no_grad():
        model.joint.b2[0] -= 0.4
        if vocab > 32:
            model.joint.W2 *= 12.0
    return model.to(DEV).eval()


def _restate(model, enc_b, max_len, f16):
    """utils/decoding.py on one utterance with a float64 joint (the f16 engine's roundings restated): ids, score, min gap."""
    jn = model.joint
    W1, b1, W2, b2 = (x.detach().cpu().numpy() for x in (jn.W1, jn.b1, jn.W2, jn.b2))
    from oracle import rnnt_oracle as orc

    hyp, score, gap = [0], 0.0, np.inf
    with torch.no_grad():
        for i in range(enc_b.shape[0]):
            while True:
                g = model.prediction(torch.tensor([hyp], device=DEV))[:, -1:, :].cpu().numpy()
                e = enc_b[None, i : i + 1].cpu().numpy()
                y = (_joint_forward_f16(e, g, W1, b1, W2, b2) if f16 else orc.joint_forward(e, g, W1, b1, W2, b2)[0])[0, 0, 0]
                top = np.sort(y)[::-1]
                gap = min(gap, float(top[0] - top[1]))
                k = int(np.argmax(y))
                score += float(y[k] - (y.max() + np.log(np.exp(y - y.max()).sum())))
                if k == 0:
                    break
                hyp.append(k)
                if len(hyp) - 1 >= max_len:
                    return hyp[1:], score, gap
    return hyp[1:], score, gap


@pytest.mark.parametrize("vocab", [12, 4096])
def test_batch_decode_matches_a_float64_restatement(vocab):
    model = _decode_model(vocab)
    torch.manual_seed(18)  # (a seed whose decisions all have clear top-2 gaps)
    B = 8
    mel = torch.randn(B, 30, 8).to(DEV)
    spec_lengths = torch.tensor([30, 25, 30, 4, 17, 30, 9, 21], device=DEV)
    ids, lengths, scores = decoding.greedy_decode_batch(model, mel, spec_lengths, max_length=40)
    assert ids.is_cuda and scores.dtype == torch.float32
    with torch.no_grad():
        enc = model.encoder(mel)
    frames = pkg.reduced_lengths(spec_lengths, model.hp.time_reduction_factor).cpu()
    min_gap = np.inf
    for b in range(B):
        want, score, gap = _restate(model, enc[b, : int(frames[b])], 40, vocab > 32)
        min_gap = min(min_gap, gap)
        n = int(lengths[b])
        assert ids[b, :n].tolist() == want, (b, ids[b, :n].tolist(), want)
        assert abs(scores[b].item() - score) <= 1e-4 * max(1.0, abs(score)), (b, scores[b].item(), score)
    assert min_gap > (1e-5 if vocab == 12 else 1e-3), "a near-tie on this seed: pick another seed"
    assert int(lengths.sum()) >= 8
    # row 0, every frame: what the one-utterance decoder emits
    ids0, len0, _ = decoding.greedy_decode_batch(model, mel[:1], None, max_length=40)
    assert ids0[0, : int(len0[0])].tolist() == decoding.greedy_decode(model, mel[:1], 40).tolist()[0]


def test_reference_defaults_at_size():
    """H = J = 640, V = 4096 (hparams.py), B = 16, 300 encoder frames: the decode finishes; two utterances against the restatement."""
    torch.manual_seed(11)
    hp = pkg.HParams(vocab_size=4096, mel_bins=4, downsample_factor=2, embedding_size=64, encoder_layers=2, encoder_size=640,
                     projection_size=640, time_reduction_index=0, pred_net_layers=1, pred_net_size=640, joint_net_size=640)
    model = pkg.Transducer(hp)
    with torch.no_grad():
        model.joint.b2[0] += 15.0  # a blank-leaning joint, as a trained one is: a few symbols per utterance
        model.joint.W2 *= 8.0
    model = model.to(DEV).eval()
    torch.manual_seed(12)
    mel = torch.randn(16, 600, 8).to(DEV)
    ids, lengths, scores = decoding.greedy_decode_batch(model, mel, max_length=60)
    torch.cuda.synchronize()
    assert decoding.LAST_STEPS >= 300 and torch.isfinite(scores).all()
    with torch.no_grad():
        enc = model.encoder(mel)
    assert enc.shape[1] == 300
    min_gap = np.inf
    for b in (0, 9):
        want, _, gap = _restate(model, enc[b], 60, True)
        min_gap = min(min_gap, gap)
        assert ids[b, : int(lengths[b])].tolist() == want, (b, ids[b, : int(lengths[b])].tolist(), want)
    assert min_gap > 1e-3, "a near-tie on this seed: pick another seed"


def test_no_host_sync_per_step(monkeypatch):
    model = _decode_model(4096)
    mel = torch.randn(6, 30, 8, device=DEV)
    with torch.no_grad():
        enc = model.encoder(mel)
    frames = torch.tensor([15, 12, 15, 3, 8, 15], dtype=torch.int32, device=DEV)
    calls = []
    real = decoding.read_flag
    monkeypatch.setattr(decoding, "read_flag", lambda x: calls.append(1) or real(x))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ids, lengths, _ = decoding.greedy_search_batch(model, enc, frames, max_length=40, check_every=4)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert decoding.LAST_STEPS % 4 == 0 and len(calls) == decoding.LAST_STEPS // 4
    ids2, lengths2, _ = decoding.greedy_search_batch(model, enc, frames, max_length=40, check_every=32)
    assert torch.equal(ids, ids2[:, : ids.shape[1]]) and torch.equal(lengths, lengths2)


def test_robustness_poisoned_and_reused_workspaces_and_done_rows(monkeypatch):
    model = _decode_model(4096)
    torch.manual_seed(5)
    mel = torch.randn(5, 30, 8, device=DEV)
    sl = torch.tensor([30, 11, 30, 6, 20], device=DEV)
    decoding._WORKSPACES.clear()
    fresh = decoding.greedy_decode_batch(model, mel, sl, max_length=40)
    decoding._WORKSPACES.clear()
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", 0xFF)  # NaN in every float word of the workspace before begin
    poisoned = decoding.greedy_decode_batch(model, mel, sl, max_length=40)
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", None)
    for a, b in zip(fresh, poisoned):
        assert torch.equal(a, b)
    # one workspace, two decodes of different shapes: the second as with a fresh workspace
    big = torch.randn(9, 40, 8, device=DEV)
    decoding.greedy_decode_batch(model, big, None, max_length=50)
    reused = decoding.greedy_decode_batch(model, mel[:3], sl[:3], max_length=40)
    decoding._WORKSPACES.clear()
    fresh3 = decoding.greedy_decode_batch(model, mel[:3], sl[:3], max_length=40)
    for a, b in zip(reused, fresh3):
        assert torch.equal(a, b)
    # finished hypotheses: further steps change nothing
    with torch.no_grad():
        enc = model.encoder(mel)
    jg = jmod.GreedyJoint(model.joint)
    jg.begin(enc, torch.tensor([15, 6, 15, 3, 10], dtype=torch.int32, device=DEV), torch.full((5,), 20, dtype=torch.int32, device=DEV), 0, 64)
    g = torch.randn(5, enc.shape[2], device=DEV)
    for _ in range(200):
        jg.step(g)
        if int(jg.all_done[0]) == 1:
            break
    assert int(jg.all_done[0]) == 1
    snap = [x.clone() for x in (jg.hyps, jg.lengths, jg.scores)]
    for _ in range(3):
        em = jg.step(g)
        assert (em == -1).all() and int(jg.all_done[0]) == 1
    for a, b in zip(snap, (jg.hyps, jg.lengths, jg.scores)):
        assert torch.equal(a, b)
