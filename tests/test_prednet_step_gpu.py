"""The prediction-network step on the MI355X (include/rnnt.h compute_rnnt_prednet_*, joint.PredictionStep): per-step parity with
a float64 restatement over chained steps with random `emitted` / `parents`, bitwise row independence and run-to-run equality,
the decoders' prediction="engine" route against the torch route and the float64 decoders, no host synchronisation per step,
poisoned and reused workspaces, and the step kernels' code object (no scratch)."""
import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import decoding, joint as jmod
from rnnt_speech_recognition_amd.joint import PredictionStep
from tests import test_beam_search_gpu as beam_gpu, test_greedy_batch_gpu as greedy_gpu
from tests.test_isa_audit import _find, kernels  # noqa: F401  (module-scoped fixture: the built code objects)

DEV = torch.device("cuda:0")

# (E, H, P, L, J): projected; unprojected; the reference defaults; odd widths (J 700 -> 704 joint units)
SHAPES = [(64, 256, 128, 2, 640), (64, 640, 640, 1, 640), (500, 2048, 640, 2, 640), (37, 200, 72, 2, 700)]
VOCAB = 64


def _net(E, H, P, L, J, seed=0):
    torch.manual_seed(seed)
    hp = pkg.HParams(vocab_size=VOCAB, embedding_size=E, pred_net_layers=L, pred_net_size=H, projection_size=P)
    net = pkg.model.PredictionNetwork(hp).eval()
    with torch.no_grad():
        for blk in net.blocks:  # non-trivial biases and LayerNorm affine parameters
            blk.lstm.bias_ih_l0.normal_(0, 0.2), blk.lstm.bias_hh_l0.normal_(0, 0.2)
            blk.norm.weight.normal_(1, 0.3), blk.norm.bias.normal_(0, 0.3)
    Jp = (J + 63) // 64 * 64
    W1 = torch.zeros(net.out_width, Jp)
    W1[:, :J] = torch.randn(net.out_width, J) / np.sqrt(net.out_width)
    return net.to(DEV), W1.to(DEV)


class _Ref:
    """The step of include/rnnt.h in float64 NumPy."""

    def __init__(self, net, W1, R):
        d = lambda x: x.detach().double().cpu().numpy()  # noqa: E731
        self.emb, self.W1 = d(net.embed.weight), d(W1)
        self.blocks = [(d(b.lstm.weight_ih_l0), d(b.lstm.weight_hh_l0), d(b.lstm.bias_ih_l0) + d(b.lstm.bias_hh_l0),
                        d(b.lstm.weight_hr_l0) if b.lstm.proj_size else None, d(b.norm.weight), d(b.norm.bias), b.norm.eps)
                       for b in net.blocks]
        self.state = [(np.zeros((R, wih.shape[0] // 4 if whr is None else whr.shape[0])), np.zeros((R, wih.shape[0] // 4)))
                      for wih, _, _, whr, _, _, _ in self.blocks]
        self.pp = np.zeros((R, W1.shape[1]))
        self.step(np.zeros(R, np.int64), None)

    def step(self, emitted, parents):
        R = len(emitted)
        src = np.arange(R) if parents is None else np.asarray(parents)
        live = np.asarray(emitted) >= 0
        x = self.emb[np.where(live, emitted, 0)]
        new = []
        for (wih, whh, b, whr, g, beta, eps), (r, c) in zip(self.blocks, self.state):
            r, c = r[src], c[src]
            z = x @ wih.T + r @ whh.T + b
            H = c.shape[1]
            sg = lambda v: 1 / (1 + np.exp(-v))  # noqa: E731
            c2 = sg(z[:, H:2 * H]) * c + sg(z[:, :H]) * np.tanh(z[:, 2 * H:3 * H])
            h = sg(z[:, 3 * H:]) * np.tanh(c2)
            r2 = h if whr is None else h @ whr.T
            new.append((np.where(live[:, None], r2, r), np.where(live[:, None], c2, c)))
            m = r2.mean(1, keepdims=True)
            x = (r2 - m) / np.sqrt(((r2 - m) ** 2).mean(1, keepdims=True) + eps) * g + beta
        self.state = new
        self.pp = np.where(live[:, None], x @ self.W1, self.pp[src])
        return self.pp


def _close(got, want):
    got = got.double().cpu().numpy()
    bar = 1e-4 * max(1.0, float(np.abs(want).max()))
    assert np.abs(got - want).max() <= bar, (np.abs(got - want).max(), bar)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "E%d_H%d_P%d_L%d_J%d" % s)
@pytest.mark.parametrize("R", [1, 16, 256])
def test_step_matches_a_float64_restatement(shape, R):
    net, W1 = _net(*shape)
    J = shape[4]
    ps = PredictionStep(net, W1)
    assert ps.engine
    ref = _Ref(net, W1, R)
    pp = ps.begin(R)
    _close(pp, ref.pp)
    rng = np.random.default_rng(R + shape[1])
    beam = 4 if R % 4 == 0 else 1
    for _ in range(32):
        emitted = rng.integers(0, VOCAB, R)
        emitted[rng.random(R) < 0.3] = -1
        parents = (np.arange(R) // beam * beam + rng.integers(0, beam, R)) if beam > 1 else None  # within the utterance
        pp = ps.step(torch.tensor(emitted, dtype=torch.int32, device=DEV),
                     None if parents is None else torch.tensor(parents, dtype=torch.int32, device=DEV))
        want = ref.step(emitted, parents)
        _close(pp, want)
        assert (pp[:, J:] == 0).all()
        for (r, c), (rr, cr) in zip(ps.state(), ref.state):
            _close(r, rr)
            _close(c, cr)


@pytest.mark.gpu
def test_rows_are_bitwise_independent_and_runs_repeat():
    net, W1 = _net(*SHAPES[0], seed=3)
    R = 256
    g = torch.Generator().manual_seed(2)
    seq = []
    for _ in range(8):
        e = torch.randint(0, VOCAB, (R,), generator=g, dtype=torch.int32)
        e[torch.rand(R, generator=g) < 0.3] = -1
        seq.append(e.to(DEV))

    def run(rows):
        ps = PredictionStep(net, W1)
        outs = [ps.begin(len(rows)).clone()]
        for e in seq:
            outs.append(ps.step(e[rows]).clone())
        return outs, [(r.clone(), c.clone()) for r, c in ps.state()]

    full, st = run(torch.arange(R, device=DEV))
    again, st2 = run(torch.arange(R, device=DEV))
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(st, st2))
    for r in (0, 37, 255):
        alone, _ = run(torch.tensor([r], device=DEV))
        assert all(torch.equal(a[0], f[r]) for a, f in zip(alone, full)), r


@pytest.mark.gpu
@pytest.mark.parametrize("vocab", [12, 4096])
@pytest.mark.parametrize("cap", [None, 1])
def test_greedy_engine_route_matches_torch_route_and_float64(vocab, cap):
    model = greedy_gpu._decode_model(vocab)
    torch.manual_seed(18)
    B = 8
    mel = torch.randn(B, 30, 8).to(DEV)
    sl = torch.tensor([30, 25, 30, 4, 17, 30, 9, 21], device=DEV)
    a = decoding.greedy_decode_batch(model, mel, sl, max_length=40, max_symbols_per_frame=cap)
    b = decoding.greedy_decode_batch(model, mel, sl, max_length=40, max_symbols_per_frame=cap, prediction="engine")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert ((a[2] - b[2]).abs() <= 1e-4 * a[2].abs().clamp(min=1)).all()
    if cap is None:
        with torch.no_grad():
            enc = model.encoder(mel)
        frames = pkg.reduced_lengths(sl, model.hp.time_reduction_factor)
        checked = 0
        for i in range(B):
            want, score, gap = greedy_gpu._restate(model, enc[i, : int(frames[i])], 40, vocab > 32)
            if gap <= 1e-3:
                continue
            checked += 1
            assert b[0][i, : int(b[1][i])].tolist() == want, i
            assert abs(b[2][i].item() - score) <= 1e-4 * max(1.0, abs(score)), i
        assert checked >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("vocab", [12, 4096])
@pytest.mark.parametrize("K", [1, 4])
def test_beam_engine_route_matches_torch_route_and_float64(vocab, K):
    model = greedy_gpu._decode_model(vocab)
    torch.manual_seed(18)
    B = 6
    mel = torch.randn(B, 24, 8).to(DEV)
    sl = torch.tensor([24, 19, 24, 4, 0, 13], device=DEV)
    with torch.no_grad():
        enc = model.encoder(mel)
    frames = pkg.reduced_lengths(sl, model.hp.time_reduction_factor)
    a = decoding.beam_search_batch(model, enc, frames, beam=K)
    ids, lengths, scores = decoding.beam_search_batch(model, enc, frames, beam=K, prediction="engine")
    assert torch.equal(a[0], ids) and torch.equal(a[1], lengths)
    fin = torch.isfinite(a[2])
    assert torch.equal(fin, torch.isfinite(scores))
    assert ((a[2][fin] - scores[fin]).abs() <= 1e-4 * a[2][fin].abs().clamp(min=1)).all()
    checked = 0
    for b in range(B):
        want, gap = beam_gpu._restate(model, enc[b, : int(frames[b])], K, vocab > 32)
        if gap <= 1e-3:
            continue
        checked += 1
        for k, (y, s) in enumerate(want):
            assert ids[b, k, : int(lengths[b, k])].tolist() == list(y), (b, k)
            assert abs(scores[b, k].item() - s) <= 1e-4 * max(1.0, abs(s)), (b, k)
    assert checked >= 2


@pytest.mark.gpu
def test_no_host_sync_per_step(monkeypatch):
    model = greedy_gpu._decode_model(4096)
    mel = torch.randn(6, 30, 8, device=DEV)
    with torch.no_grad():
        enc = model.encoder(mel)
    frames = torch.tensor([15, 12, 15, 3, 8, 15], dtype=torch.int32, device=DEV)
    decoding.greedy_search_batch(model, enc, frames, max_length=40, prediction="engine")  # (allocations)
    decoding.beam_search_batch(model, enc, frames, beam=4, prediction="engine")
    calls = []
    real = decoding.read_flag
    monkeypatch.setattr(decoding, "read_flag", lambda x: calls.append(1) or real(x))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ids, lengths, _ = decoding.greedy_search_batch(model, enc, frames, max_length=40, check_every=4, prediction="engine")
        beam = decoding.beam_search_batch(model, enc, frames, beam=4, prediction="engine")
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert decoding.LAST_STEPS % 4 == 0 and len(calls) == decoding.LAST_STEPS // 4
    ref = decoding.greedy_search_batch(model, enc, frames, max_length=40, check_every=4)
    assert torch.equal(ids, ref[0]) and torch.equal(lengths, ref[1])
    assert torch.equal(beam[0], decoding.beam_search_batch(model, enc, frames, beam=4)[0])


@pytest.mark.gpu
def test_poisoned_and_reused_workspaces(monkeypatch):
    net, W1 = _net(*SHAPES[0], seed=4)
    g = torch.Generator().manual_seed(9)
    R = 16
    seq = [(torch.randint(-1, VOCAB, (R,), generator=g, dtype=torch.int32).to(DEV),
            torch.randint(0, R, (R,), generator=g, dtype=torch.int32).to(DEV)) for _ in range(6)]

    def run(ws=None):
        ps = PredictionStep(net, W1)
        ps._ws = ws
        outs = [ps.begin(R).clone()]
        outs += [ps.step(e, p).clone() for e, p in seq]
        return outs, ps._ws

    fresh, _ = run()
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", 0xFF)  # NaN in every float word of the workspace before begin
    poisoned, _ = run()
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", None)
    big = PredictionStep(net, W1)
    big.begin(300)
    big.step(torch.zeros(300, dtype=torch.int32, device=DEV))
    reused, ws = run(big._ws)
    assert ws is big._ws
    for a, b, c in zip(fresh, poisoned, reused):
        assert torch.equal(a, b) and torch.equal(a, c)
    model = greedy_gpu._decode_model(4096)
    mel = torch.randn(5, 30, 8, device=DEV)
    sl = torch.tensor([30, 11, 30, 6, 20], device=DEV)
    decoding._PRED_WORKSPACES.clear()
    want = decoding.greedy_decode_batch(model, mel, sl, max_length=40, prediction="engine")
    decoding._PRED_WORKSPACES.clear()
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", 0xFF)
    got = decoding.greedy_decode_batch(model, mel, sl, max_length=40, prediction="engine")
    assert all(torch.equal(x, y) for x, y in zip(want, got))


def test_step_kernels_use_no_scratch(kernels):
    meta, _ = kernels
    names = _find(meta, "prednet_kernel")
    assert len(names) == 15
    for k in names + _find(meta, "prednet_pack_kernel"):
        assert int(meta[k]["private_segment_fixed_size"]) == 0, k
        assert int(meta[k].get("vgpr_spill_count", "0")) == 0, k
