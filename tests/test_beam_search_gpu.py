"""Batched beam search on an MI355X: the step's per-hypothesis top-K and logsumexp against compute_rnnt_joint_logits (bitwise
logits), the whole decode against a float64 restatement, beam = 1 against greedy, the reference's defaults at size, no host
sync per step, robustness of the workspace."""
import math

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib, decoding, joint as jmod
from tests.test_frontend import _joint_forward_f16, small_model
from tests.test_greedy_batch_gpu import STEP_CASES, _decode_model, _ref_logits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

BEAM_STEP_CASES = [c for c in STEP_CASES if c[2] != 1000] + [(1, 256, 1000), (0, 704, 28)]


def _opts(blank, T):
    return _lib.make_options(torch.cuda.current_stream().cuda_stream, blank, T, 1)


@pytest.mark.parametrize("case", range(len(BEAM_STEP_CASES)))
def test_step_topk_matches_the_logits_entry_per_hypothesis(case):
    dtype, J, V = BEAM_STEP_CASES[case]
    K = (1, 4, 16)[case % 3]
    B = (3, 9, 2, 5)[case % 4]  # B K: 3, 36, 32, 80 ... (not all multiples of 32)
    T = 4
    g = torch.Generator().manual_seed(2000 + case)
    enc = torch.randn(B, T, J, generator=g)
    pred = torch.randn(B * K, J, generator=g)
    if B * K > 2:  # one enc row and one pred row beyond the e^{2x} table range
        enc[1 % B, 0] *= 60.0
        pred[2] *= 60.0
    W2 = torch.rand(J, V, generator=g) * 2 - 1
    W2 *= (6.0 / (J + V)) ** 0.5 * (3.0 if dtype == 0 else 12.0)
    b2 = 0.1 * torch.randn(V, generator=g)
    enc, pred, W2, b2 = (x.to(DEV).contiguous() for x in (enc, pred, W2, b2))
    R = B * K
    frames = torch.full((B,), T, dtype=torch.int32, device=DEV)
    ws = torch.empty(_lib.beam_workspace_bytes(T, B, K, J, V, dtype), dtype=torch.uint8, device=DEV)
    parents, emitted = (torch.zeros(R, dtype=torch.int32, device=DEV) for _ in range(2))
    tl = torch.full((R, K), float("nan"), device=DEV)
    ts = torch.full((R, K), -7, dtype=torch.int32, device=DEV)
    lse = torch.full((R,), float("nan"), device=DEV)
    lib = _lib.load()
    _lib.check(lib.compute_rnnt_beam_begin(enc.data_ptr(), frames.data_ptr(), W2.data_ptr(), b2.data_ptr(), J, V, B, K, dtype,
                                           ws.data_ptr(), _opts(0, T)), "begin")
    # step 1: only slot 0 of each beam is live; step 2: every slot the first step filled
    for step in range(2):
        if step == 0:
            live = [b * K for b in range(B)]
        else:
            hl = torch.empty(B, K, T, dtype=torch.int32, device=DEV)
            ln = torch.empty(B, K, dtype=torch.int32, device=DEV)
            sc = torch.empty(B, K, device=DEV)
            _lib.check(lib.compute_rnnt_beam_results(hl.data_ptr(), ln.data_ptr(), sc.data_ptr(), J, V, B, K, dtype, ws.data_ptr(),
                                                     _opts(0, T)), "results")
            torch.cuda.synchronize()
            live = [b * K + k for b in range(B) for k in range(K) if math.isfinite(sc[b, k].item())]
            assert len(live) == B * min(K, V)
        _lib.check(lib.compute_rnnt_beam_step(pred.data_ptr(), parents.data_ptr(), emitted.data_ptr(), tl.data_ptr(), ts.data_ptr(),
                                              lse.data_ptr(), J, V, B, K, dtype, ws.data_ptr(), _opts(0, T)), "step")
        torch.cuda.synchronize()
        if step == 0:
            for b in range(B):
                assert parents[b * K : (b + 1) * K].tolist()[: min(K, V)] == [b * K] * min(K, V)
        tl_c, ts_c, lse_c = tl.cpu(), ts.cpu(), lse.cpu()
        for r in live:
            ref = _ref_logits(enc[r // K, step].contiguous(), pred[r].contiguous(), W2, b2, dtype)[:V].cpu()
            order = sorted(range(V), key=lambda v: (-ref[v].item(), v))[:K]
            n = min(K, V)
            assert ts_c[r, :n].tolist() == order, (case, step, r)
            if dtype == 0 and J > 640:  # DT 2 (J = 704): the shared joint sits ~1e-7 off the logits entry on a few symbols
                assert ((tl_c[r, :n] - ref[order]).abs() <= 1e-6 * ref[order].abs().clamp(min=1.0)).all(), (case, step, r)
            else:
                assert torch.equal(tl_c[r, :n], ref[order]), (case, step, r)  # bitwise
            if n < K:
                assert (ts_c[r, n:] == -1).all()
            want = float(torch.logsumexp(ref.double(), 0))
            assert abs(lse_c[r].item() - want) <= 1e-6 * max(1.0, abs(want)), (case, step, r, lse_c[r].item(), want)


def _restate(model, enc_b, K, f16):
    """The algorithm of include/rnnt.h on one utterance with a float64 joint (f16: the binary16 roundings restated) -> n-best,
    smallest score gap among the first K + 1 ranked candidates."""
    jn = model.joint
    W1, b1, W2, b2 = (x.detach().cpu().numpy() for x in (jn.W1, jn.b1, jn.W2, jn.b2))
    from oracle import rnnt_oracle as orc

    beam, gap = [((), 0.0)], math.inf
    with torch.no_grad():
        for i in range(enc_b.shape[0]):
            e = enc_b[None, i : i + 1].cpu().numpy()
            cands = []
            for hi, (y, s) in enumerate(beam):
                g = model.prediction(torch.tensor([(0,) + y], device=DEV))[:, -1:, :].cpu().numpy()
                lg = (_joint_forward_f16(e, g, W1, b1, W2, b2) if f16 else orc.joint_forward(e, g, W1, b1, W2, b2)[0])[0, 0, 0]
                lse = lg.max() + np.log(np.exp(lg - lg.max()).sum())
                top = np.argsort(-lg, kind="stable")[: K + 1]
                cands += [(s + float(lg[v] - lse), hi, int(v)) for v in top]
            cands.sort(key=lambda c: (-c[0], c[1], c[2]))
            sc = [c[0] for c in cands[: K + 1]]
            gap = min([gap] + [a - b for a, b in zip(sc, sc[1:])])
            merged, order = {}, []
            for s, hi, v in cands[:K]:
                y = beam[hi][0] if v == 0 else beam[hi][0] + (v,)
                if y in merged:
                    a = merged[y]
                    merged[y] = max(a, s) + math.log1p(math.exp(min(a, s) - max(a, s)))
                else:
                    merged[y], order = s, order + [y]
            beam = sorted(((y, merged[y]) for y in order), key=lambda e: -e[1])
    return beam, gap


@pytest.mark.parametrize("vocab,K", [(12, 4), (28, 8), (256, 4), (4096, 4)])
def test_beam_decode_matches_a_float64_restatement(vocab, K):
    model = _decode_model(vocab)
    torch.manual_seed(18)
    B = 6
    mel = torch.randn(B, 24, 8).to(DEV)
    spec_lengths = torch.tensor([24, 19, 24, 4, 0, 13], device=DEV)
    with torch.no_grad():
        enc = model.encoder(mel)
    frames = pkg.reduced_lengths(spec_lengths, model.hp.time_reduction_factor)
    ids, lengths, scores = decoding.beam_search_batch(model, enc, frames, beam=K)
    assert ids.is_cuda and scores.dtype == torch.float32
    margin = 1e-5 if vocab <= 32 else 1e-3
    checked = 0
    for b in range(B):
        want, gap = _restate(model, enc[b, : int(frames[b])], K, vocab > 32)
        if gap <= margin:
            continue  # a near-tie: the f32 engine may rank it either way
        checked += 1
        for k, (y, s) in enumerate(want):
            n = int(lengths[b, k])
            assert ids[b, k, :n].tolist() == list(y), (vocab, b, k)
            assert abs(scores[b, k].item() - s) <= 1e-4 * max(1.0, abs(s)), (vocab, b, k, scores[b, k].item(), s)
        assert (lengths[b, len(want):] == 0).all()
    assert checked >= 3, "too many near-ties on this seed: pick another seed"
    best = decoding.beam_decode_batch(model, mel, spec_lengths, beam=K)
    assert torch.equal(best[0], ids[:, 0]) and torch.equal(best[1], lengths[:, 0]) and torch.equal(best[2], scores[:, 0])


@pytest.mark.parametrize("vocab", [12, 4096])
def test_beam_one_is_greedy_on_the_engine(vocab):
    model = _decode_model(vocab)
    torch.manual_seed(3)
    mel = torch.randn(7, 30, 8, device=DEV)
    with torch.no_grad():
        enc = model.encoder(mel)
    frames = torch.tensor([15, 12, 0, 3, 8, 15, 15], dtype=torch.int32, device=DEV)
    ids, lengths, scores = decoding.beam_search_batch(model, enc, frames, beam=1)
    gids, glen, gsc = decoding.greedy_search_batch(model, enc, frames, None, 1)
    assert torch.equal(lengths[:, 0], glen)
    for b in range(7):
        n = int(glen[b])
        assert ids[b, 0, :n].tolist() == gids[b, :n].tolist()
        s = gsc[b].item()
        assert abs(scores[b, 0].item() - s) <= 1e-6 * max(1.0, abs(s))


def test_reference_defaults_at_size():
    torch.manual_seed(11)
    hp = pkg.HParams(vocab_size=4096, mel_bins=4, downsample_factor=2, embedding_size=64, encoder_layers=2, encoder_size=640,
                     projection_size=640, time_reduction_index=0, pred_net_layers=1, pred_net_size=640, joint_net_size=640)
    model = pkg.Transducer(hp)
    with torch.no_grad():
        model.joint.b2[0] += 15.0
        model.joint.W2 *= 8.0
    model = model.to(DEV).eval()
    torch.manual_seed(12)
    mel = torch.randn(16, 600, 8).to(DEV)
    with torch.no_grad():
        enc = model.encoder(mel)
    assert enc.shape[1] == 300
    frames = torch.full((16,), 300, dtype=torch.int32, device=DEV)
    one = decoding.beam_search_batch(model, enc, frames, beam=4)
    two = decoding.beam_search_batch(model, enc, frames, beam=4)
    torch.cuda.synchronize()
    ids, lengths, scores = one
    assert torch.isfinite(scores[:, 0]).all()
    s = scores.double().nan_to_num(neginf=-1e300)
    assert (s[:, 1:] <= s[:, :-1]).all()
    for a, b in zip(one, two):
        assert torch.equal(a, b)


def test_no_host_sync_per_step():
    model = _decode_model(4096)
    mel = torch.randn(6, 30, 8, device=DEV)
    with torch.no_grad():
        enc = model.encoder(mel)
    frames = torch.tensor([15, 12, 15, 3, 8, 15], dtype=torch.int32, device=DEV)
    decoding.beam_search_batch(model, enc, frames, beam=4)  # (allocations)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = decoding.beam_search_batch(model, enc, frames, beam=4)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    ref = decoding.beam_search_batch(model, enc, frames, beam=4)
    for a, b in zip(out, ref):
        assert torch.equal(a, b)


def test_robustness_poisoned_and_reused_workspaces(monkeypatch):
    model = _decode_model(4096)
    torch.manual_seed(5)
    mel = torch.randn(5, 30, 8, device=DEV)
    sl = torch.tensor([30, 11, 30, 6, 20], device=DEV)
    decoding._BEAM_WORKSPACES.clear()
    fresh = decoding.beam_decode_batch(model, mel, sl, beam=4)
    decoding._BEAM_WORKSPACES.clear()
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", 0xFF)  # NaN in every float word of the workspace before begin
    poisoned = decoding.beam_decode_batch(model, mel, sl, beam=4)
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", None)
    for a, b in zip(fresh, poisoned):
        assert torch.equal(a, b)
    big = torch.randn(9, 40, 8, device=DEV)
    decoding.beam_decode_batch(model, big, None, beam=8)
    reused = decoding.beam_decode_batch(model, mel[:3], sl[:3], beam=4)
    decoding._BEAM_WORKSPACES.clear()
    fresh3 = decoding.beam_decode_batch(model, mel[:3], sl[:3], beam=4)
    for a, b in zip(reused, fresh3):
        assert torch.equal(a, b)
