"""The encoder's forward pass on the MI355X (include/rnnt.h compute_rnnt_encoder_*, joint.EncoderStream): parity of the output
and of every block's state with a float64 restatement, bitwise row independence, chunked runs against one run, run-to-run
equality, the decoders' encoder="engine" route against the torch route, no host synchronisation per run, poisoned and reused
workspaces, and the kernels' code object (no scratch, no spills)."""
import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import decoding, joint as jmod
from rnnt_speech_recognition_amd.joint import EncoderStream
from tests import test_greedy_batch_gpu as greedy_gpu
from tests.test_isa_audit import _find, kernels  # noqa: F401  (module-scoped fixture: the built code objects)

DEV = torch.device("cuda:0")

# (feat = mel x downsample, H, P, layers, reduction index, factor, frames, rows): small projected; unprojected (configs[2]-like,
# 2 x 320); the reference defaults (8 x 2048 / 640); odd widths
SHAPES = {
    "small": ((4, 3), 256, 128, 3, 1, 2, 37, (1, 16, 64)),
    "unproj": ((80, 3), 320, 320, 2, 0, 2, 61, (1, 16, 64)),
    "ref": ((80, 3), 2048, 640, 8, 1, 2, 201, (4,)),
    "odd": ((13, 1), 200, 72, 3, 1, 3, 29, (1, 16, 64)),
}


def _encoder(feat, H, P, L, ridx, f, seed=0):
    torch.manual_seed(seed)
    hp = pkg.HParams(mel_bins=feat[0], downsample_factor=feat[1], encoder_layers=L, encoder_size=H, projection_size=P,
                     time_reduction_index=ridx, time_reduction_factor=f)
    enc = pkg.model.Encoder(hp)
    with torch.no_grad():  # non-trivial running statistics, biases and LayerNorm affine parameters
        bn = enc.input_norm
        bn.running_mean.normal_(0, 0.5), bn.running_var.uniform_(0.5, 2.0), bn.weight.normal_(1, 0.2), bn.bias.normal_(0, 0.2)
        for blk in enc.blocks:
            blk.lstm.bias_ih_l0.normal_(0, 0.2), blk.lstm.bias_hh_l0.normal_(0, 0.2)
            blk.norm.weight.normal_(1, 0.3), blk.norm.bias.normal_(0, 0.3)
    return enc.to(DEV).eval()


def _restate(enc, x):
    """model.Encoder.forward (eval) in float64 NumPy, one run from zero state -> (out, [(r, c) per block])."""
    d = lambda t: t.detach().double().cpu().numpy()  # noqa: E731
    sg = lambda v: 1 / (1 + np.exp(-v))  # noqa: E731
    bn = enc.input_norm
    h = (d(x) - d(bn.running_mean)) / np.sqrt(d(bn.running_var) + bn.eps) * d(bn.weight) + d(bn.bias)
    states = []
    for i, blk in enumerate(enc.blocks):
        lstm, norm = blk.lstm, blk.norm
        H = lstm.hidden_size
        whh, whr = d(lstm.weight_hh_l0), (d(lstm.weight_hr_l0) if lstm.proj_size else None)
        pre = h @ d(lstm.weight_ih_l0).T + d(lstm.bias_ih_l0) + d(lstm.bias_hh_l0)
        R, T = h.shape[0], h.shape[1]
        r, c = np.zeros((R, whh.shape[1])), np.zeros((R, H))
        ys = np.empty((R, T, whh.shape[1]))
        for t in range(T):
            z = pre[:, t] + r @ whh.T
            c = sg(z[:, H:2 * H]) * c + sg(z[:, :H]) * np.tanh(z[:, 2 * H:3 * H])
            hh = sg(z[:, 3 * H:]) * np.tanh(c)
            r = hh if whr is None else hh @ whr.T
            ys[:, t] = r
        states.append((r, c))
        m = ys.mean(-1, keepdims=True)
        h = (ys - m) / np.sqrt(((ys - m) ** 2).mean(-1, keepdims=True) + norm.eps) * d(norm.weight) + d(norm.bias)
        if i == enc.reduction_index:
            f = enc.reduce.factor
            pad = (-T) % f
            h = np.concatenate([h, np.zeros((R, pad, h.shape[2]))], axis=1).reshape(R, (T + pad) // f, -1)
    return h, states


def _close(got, want):
    got = got.double().cpu().numpy()
    bar = 1e-4 * max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    assert err <= bar, (err, bar)


def _cases():
    for name, s in SHAPES.items():
        for R in s[7]:
            yield pytest.param(name, R, id=f"{name}_R{R}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,R", list(_cases()))
def test_run_matches_a_float64_restatement(name, R):
    feat, H, P, L, ridx, f, T, _ = SHAPES[name]
    enc = _encoder(feat, H, P, L, ridx, f, seed=R)
    es = EncoderStream(enc)
    assert es.engine
    torch.manual_seed(100 + R)
    x = torch.randn(R, T, feat[0] * feat[1], device=DEV)
    es.begin(R, T)
    out = es.run(x)
    want, states = _restate(enc, x)
    assert out.shape == want.shape
    _close(out, want)
    for (r, c), (rr, cr) in zip(es.state(), states):
        _close(r, rr)
        _close(c, cr)
    with torch.no_grad():  # and the module itself, at the same bar
        _close(out, enc(x).double().cpu().numpy())


def _run(enc, x, chunks=None, ws=None):
    es = EncoderStream(enc)
    es._ws = ws
    es.begin(x.shape[0], x.shape[1])
    bounds = [0] + list(chunks or []) + [x.shape[1]]
    out = torch.cat([es.run(x[:, a:b]) for a, b in zip(bounds[:-1], bounds[1:])], dim=1)
    return out, [(r.clone(), c.clone()) for r, c in es.state()], es._ws


def _same(a, b):
    return torch.equal(a[0], b[0]) and all(torch.equal(p, q) and torch.equal(s, t) for (p, s), (q, t) in zip(a[1], b[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "unproj", "odd"])
def test_rows_are_bitwise_independent_chunks_and_runs_repeat(name):
    feat, H, P, L, ridx, f, T, _ = SHAPES[name]
    enc = _encoder(feat, H, P, L, ridx, f, seed=5)
    R = 16
    torch.manual_seed(6)
    x = torch.randn(R, T, feat[0] * feat[1], device=DEV)
    full = _run(enc, x)
    assert _same(full, _run(enc, x))
    perm = torch.randperm(R, device=DEV)
    shuffled = _run(enc, x[perm])
    assert torch.equal(shuffled[0], full[0][perm])
    for (r, c), (r2, c2) in zip(full[1], shuffled[1]):
        assert torch.equal(r2, r[perm]) and torch.equal(c2, c[perm])
    for row in (0, 7, 15):
        alone = _run(enc, x[row: row + 1])
        assert torch.equal(alone[0][0], full[0][row]), row
        assert all(torch.equal(r[0], rf[row]) and torch.equal(c[0], cf[row]) for (r, c), (rf, cf) in zip(alone[1], full[1])), row
    cuts = [2 * f, 5 * f, 9 * f]  # multiples of f, then the odd tail
    assert _same(full, _run(enc, x, cuts))
    assert _same(full, _run(enc, x, [f * (T // f)]))


@pytest.mark.gpu
@pytest.mark.parametrize("vocab", [12, 4096])
@pytest.mark.parametrize("prediction", ["torch", "engine"])
def test_decoders_with_the_engine_encoder_match_the_torch_encoder(vocab, prediction):
    model = greedy_gpu._decode_model(vocab)
    torch.manual_seed(18)
    B = 8
    mel = torch.randn(B, 30, 8).to(DEV)
    sl = torch.tensor([30, 25, 30, 4, 17, 30, 9, 21], device=DEV)
    a = decoding.greedy_decode_batch(model, mel, sl, max_length=40, prediction=prediction)
    b = decoding.greedy_decode_batch(model, mel, sl, max_length=40, prediction=prediction, encoder="engine")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert ((a[2] - b[2]).abs() <= 1e-4 * a[2].abs().clamp(min=1)).all()
    for K in (1, 4):
        a = decoding.beam_decode_batch(model, mel, sl, beam=K, prediction=prediction)
        b = decoding.beam_decode_batch(model, mel, sl, beam=K, prediction=prediction, encoder="engine")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), K
        fin = torch.isfinite(a[2])
        assert torch.equal(fin, torch.isfinite(b[2]))
        assert ((a[2][fin] - b[2][fin]).abs() <= 1e-4 * a[2][fin].abs().clamp(min=1)).all(), K


@pytest.mark.gpu
def test_no_host_sync_per_run():
    enc = _encoder(*SHAPES["small"][:6], seed=8)
    x = torch.randn(16, 40, 12, device=DEV)
    es = EncoderStream(enc)
    es.begin(16, 20)
    es.run(x[:, :20])  # (allocations)
    es.begin(16, 20)
    want = torch.cat([es.run(x[:, :20]), es.run(x[:, 20:])], dim=1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        es.begin(16, 20)
        got = torch.cat([es.run(x[:, :20]), es.run(x[:, 20:])], dim=1)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_poisoned_and_reused_workspaces(monkeypatch):
    enc = _encoder(*SHAPES["small"][:6], seed=9)
    x = torch.randn(16, 37, 12, device=DEV)
    fresh = _run(enc, x, [6])
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", 0xFF)  # NaN in every float word of the workspace before begin
    poisoned = _run(enc, x, [6])
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", None)
    big = _run(enc, torch.randn(64, 90, 12, device=DEV))
    reused = _run(enc, x, [6], ws=big[2])
    assert reused[2] is big[2]
    assert _same(fresh, poisoned) and _same(fresh, reused)
    model = greedy_gpu._decode_model(4096)
    mel = torch.randn(5, 30, 8, device=DEV)
    sl = torch.tensor([30, 11, 30, 6, 20], device=DEV)
    decoding._ENC_WORKSPACES.clear()
    want = decoding.greedy_decode_batch(model, mel, sl, max_length=40, encoder="engine", prediction="engine")
    decoding._ENC_WORKSPACES.clear()
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", 0xFF)
    got = decoding.greedy_decode_batch(model, mel, sl, max_length=40, encoder="engine", prediction="engine")
    assert all(torch.equal(p, q) for p, q in zip(want, got))


def test_encoder_kernels_use_no_scratch(kernels):
    meta, _ = kernels
    names = _find(meta, "enc_step_kernel")
    assert len(names) == 10
    for k in names + _find(meta, "enc_gemm_kernel") + _find(meta, "enc_norm_kernel") + _find(meta, "encoder_pack_kernel"):
        assert int(meta[k]["private_segment_fixed_size"]) == 0, k
        assert int(meta[k].get("vgpr_spill_count", "0")) == 0, k
