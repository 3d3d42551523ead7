"""Streaming greedy decoding on the MI355X (decoding.StreamingGreedyDecoder over compute_rnnt_encoder_run_rows,
compute_rnnt_prednet_reset and compute_rnnt_greedy_stream_*): streams against the float64 restatement, bitwise equality of a
stream in one slot and in slot k of 16 under other traffic, equality with greedy_decode_batch, the ragged encoder run and the
prediction-network reset bit for bit, the reference defaults at size, no host sync per step, poisoned and reused workspaces,
and no scratch in the new kernels."""
import random

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import decoding, joint as jmod
from rnnt_speech_recognition_amd.decoding import StreamingGreedyDecoder
from rnnt_speech_recognition_amd.joint import EncoderStream, PredictionStep
from tests import test_greedy_batch_gpu as greedy_gpu
from tests.test_encoder_stream_gpu import SHAPES, _encoder
from tests.test_isa_audit import _find, kernels  # noqa: F401  (module-scoped fixture: the built code objects)
from tests.test_streaming_greedy import chunkings, one_call, run_schedule

DEV = torch.device("cuda:0")


def _streams(F, lengths, seed):
    torch.manual_seed(seed)
    return [torch.randn(L, F, device=DEV) for L in lengths]


def _schedule(lengths, f, kind, seed, slots=None):
    rng = random.Random(seed)
    slots = slots or list(range(len(lengths)))
    return [(slots[i], i % 4, chunkings(L, f, rng)[kind]) for i, L in enumerate(lengths)]


@pytest.mark.gpu
@pytest.mark.parametrize("vocab", [12, 4096])
def test_streams_match_a_float64_restatement(vocab):
    model = greedy_gpu._decode_model(vocab)
    f = model.encoder.reduce.factor
    lengths = [30, 25, 17, 9, 22, 30]
    X = _streams(8, lengths, 18)
    plans = _schedule(lengths, f, "random", 3, slots=[5, 0, 3, 1, 4, 2])
    got, emitted = run_schedule(model, X, 6, max(max(p[2]) for p in plans), plans, 40)
    assert decoding.StreamingGreedyDecoder(model, 1, 8).gj.engine
    min_gap, total = np.inf, 0
    for i, x in enumerate(X):
        with torch.no_grad():
            enc = model.encoder(x[None])[0]
        want, score, gap = greedy_gpu._restate(model, enc, 40, vocab > 32)
        min_gap = min(min_gap, gap)
        ids, n, sc = got[i]
        assert ids == want and emitted[i] == want, (i, ids, want)
        assert abs(float(sc) - score) <= 1e-4 * max(1.0, abs(score)), (i, float(sc), score)
        total += n
    assert min_gap > (1e-5 if vocab == 12 else 1e-3), "a near-tie on this seed: pick another seed"
    assert total >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("vocab", [12, 4096])
def test_one_slot_and_slot_k_of_16_are_bitwise_equal(vocab):
    model = greedy_gpu._decode_model(vocab)
    f = model.encoder.reduce.factor
    lengths = [30, 24, 11, 28, 17, 30, 5, 22, 19, 26, 13, 30]
    X = _streams(8, lengths, 21)
    want = [one_call(model, x, 40) for x in X]
    for i, x in enumerate(X[:4]):  # property 2: the ids of greedy_decode_batch of the stream alone
        bi, bl, _ = decoding.greedy_decode_batch(model, x[None], None, 40)
        assert bi[0, : int(bl[0])].tolist() == want[i][0], i
    slots = [15, 3, 7, 0, 9, 12, 1, 4, 14, 6, 10, 2]
    for kind in ["one", "f", "random"]:
        plans = _schedule(lengths, f, kind, 5, slots)
        Tc = max(max(p[2]) for p in plans)
        got, emitted = run_schedule(model, X, 16, Tc, plans, 40, seed=len(kind), extra_restart=(1, 11))
        for i in range(len(X)):
            ids, n, sc = got[i]
            assert ids == want[i][0] and n == want[i][1] and emitted[i] == ids, (kind, i)
            assert torch.equal(sc, want[i][2]), (kind, i, float(sc), float(want[i][2]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "odd"])
def test_encoder_run_rows_is_bitwise_a_row_run_alone(name):
    feat, H, P, L, ridx, f = SHAPES[name][:6]
    enc = _encoder(feat, H, P, L, ridx, f, seed=4)
    R, F, T = 6, feat[0] * feat[1], 4 * f
    x = torch.randn(R, 3 * T, F, device=DEV)
    es = EncoderStream(enc)
    assert es.engine
    es.begin(R, T)
    es.run(x[:, :T])
    before = [(h.clone(), c.clone()) for h, c in es.state()]
    rows = [T, 0, T - 1, f, 0, 1]
    reset = [False, False, True, False, True, False]
    out = es.run(x[:, T: 2 * T], row_frames=rows, reset=reset)
    st = es.state()
    for r in range(R):
        one = EncoderStream(enc)
        one.begin(1, T)
        if not reset[r]:
            one.run(x[r: r + 1, :T])
        ref = [(h.clone(), c.clone()) for h, c in one.state()]
        if rows[r]:
            w = one.run(x[r: r + 1, T: T + rows[r]])
            assert torch.equal(out[r: r + 1, : w.shape[1]], w), r
            assert not out[r, w.shape[1]:].any(), r
            ref = one.state()
        elif not reset[r]:
            ref = [(h[r: r + 1], c[r: r + 1]) for h, c in before]
        for (h, c), (h1, c1) in zip(st, ref):
            assert torch.equal(h[r], h1[0]) and torch.equal(c[r], c1[0]), r
    # no rows and no reset: the plain run, bit for bit
    a, b = EncoderStream(enc), EncoderStream(enc)
    a.begin(R, T), b.begin(R, T)
    assert torch.equal(a.run(x[:, :T]), b.run(x[:, :T], row_frames=[T] * R))
    assert all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) for p, q in zip(a.state(), b.state()))


@pytest.mark.gpu
@pytest.mark.parametrize("parents", [False, True])
def test_prednet_reset_is_bitwise_a_fresh_begin(parents):
    model = greedy_gpu._decode_model(4096)
    gj = jmod.GreedyJoint(model.joint)
    R = 8
    ps, fresh = PredictionStep(model.prediction, gj.W1), PredictionStep(model.prediction, gj.W1)
    assert ps.engine
    f0 = fresh.begin(R).clone()
    ps.begin(R)
    ps.step(torch.tensor([3, -1, 5, 2, 7, 1, -1, 9], dtype=torch.int32, device=DEV))
    moved = ps.step(torch.tensor([1, 4, -1, 2, 6, -1, 3, 8], dtype=torch.int32, device=DEV)).clone()
    m = [True, False, False, True, False, True, False, False]
    pp = ps.reset(m).clone()
    for r in range(R):
        assert torch.equal(pp[r], f0[r] if m[r] else moved[r]), r
    for (h, c), (h0, c0) in zip(ps.state(), fresh.state()):
        for r in range(R):
            if m[r]:
                assert torch.equal(h[r], h0[r]) and torch.equal(c[r], c0[r])
    em = torch.tensor([2, 5, -1, 4, 1, 3, -1, 6], dtype=torch.int32, device=DEV)
    pa = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7], dtype=torch.int32, device=DEV) if parents else None
    got = ps.step(em, pa).clone()
    ctrl = PredictionStep(model.prediction, gj.W1)  # the same history without the reset: the carried rows agree
    ctrl.begin(R)
    ctrl.step(torch.tensor([3, -1, 5, 2, 7, 1, -1, 9], dtype=torch.int32, device=DEV))
    ctrl.step(torch.tensor([1, 4, -1, 2, 6, -1, 3, 8], dtype=torch.int32, device=DEV))
    want = ctrl.step(em, pa)
    for r in range(R):
        if not m[r]:
            assert torch.equal(got[r], want[r]), r


@pytest.mark.gpu
def test_reference_defaults_at_size():
    """The reference defaults (H = J = 640, V = 4096, the 8 x 2048 / 640 encoder, the 2 x 2048 / 640 prediction network), 16
    slots, chunks of 16 frames: two streams against the restatement."""
    torch.manual_seed(11)
    hp = pkg.HParams()  # (the reference defaults)
    model = pkg.Transducer(hp)
    with torch.no_grad():
        model.joint.b2[0] += 15.0  # a blank-leaning joint, as a trained one is: a few symbols per stream
        model.joint.W2 *= 8.0
    model = model.to(DEV).eval()
    S, Tc = 16, 16
    X = _streams(240, [96, 80], 12)
    dec = StreamingGreedyDecoder(model, S, Tc, max_length=60)
    assert dec.es._use_engine and dec.gj.engine and dec.ps._use_engine
    dec.start(list(range(S)))
    noise = torch.randn(S, 96, 240, device=DEV)
    for k in range(6):
        mel = noise[:, 16 * k: 16 * k + 16].clone()
        mel[3, :] = X[0][16 * k: 16 * k + 16]
        frames, final = [Tc] * S, [k == 5] * S
        if k < 5:
            mel[11, :] = X[1][16 * k: 16 * k + 16]
        else:
            frames[11] = 0
        final[11] = k == 4
        dec.feed(mel, frames, final)
    ids, lengths, scores = dec.hypotheses()
    assert torch.isfinite(scores).all()
    min_gap = np.inf
    for slot, x in ((3, X[0]), (11, X[1])):
        with torch.no_grad():
            enc = model.encoder(x[None])[0]
        want, _, gap = greedy_gpu._restate(model, enc, 60, True)
        min_gap = min(min_gap, gap)
        assert ids[slot, : int(lengths[slot])].tolist() == want, (slot, ids[slot, : int(lengths[slot])].tolist(), want)
    assert min_gap > 1e-3, "a near-tie on this seed: pick another seed"


@pytest.mark.gpu
def test_no_host_sync_per_step(monkeypatch):
    model = greedy_gpu._decode_model(4096)
    X = _streams(8, [40, 40, 40, 40], 6)
    dec = StreamingGreedyDecoder(model, 4, 20, max_symbols_per_frame=2, check_every=4)  # (no budget: never finished early)
    dec.start([0, 1, 2, 3])
    dec.feed(torch.stack([x[:20] for x in X]), [20] * 4, [False] * 4)  # (allocations)
    calls = []
    real = decoding.read_flag
    monkeypatch.setattr(decoding, "read_flag", lambda x: calls.append(1) or real(x))
    decoding.LAST_STEPS = 0
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        dec.feed(torch.stack([x[20:] for x in X]), [20] * 4, [True] * 4)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    steps = decoding.LAST_STEPS
    assert steps >= 10
    assert len(calls) == steps // 4 + 1  # the all-done word every check_every steps, then N once


def _decode_all(model, X, ws=None):
    dec = StreamingGreedyDecoder(model, len(X), 10, max_length=40, check_every=4)
    if ws is not None:
        dec.gj._ws = ws
        dec.gj.begin(len(X), dec.Te, 0, 40)
    dec.start(list(range(len(X))))
    for k in range(3):
        dec.feed(torch.stack([x[10 * k: 10 * k + 10] for x in X]), [10] * len(X), [k == 2] * len(X))
    return dec.hypotheses(), dec.gj._ws


@pytest.mark.gpu
def test_poisoned_and_reused_workspaces(monkeypatch):
    model = greedy_gpu._decode_model(4096)
    X = _streams(8, [30] * 5, 9)
    fresh, _ = _decode_all(model, X)
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", 0xFF)  # NaN in every float word of the workspaces before begin
    poisoned, _ = _decode_all(model, X)
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", None)
    _, big = _decode_all(model, _streams(8, [30] * 64, 10))
    reused, ws = _decode_all(model, X, ws=big)
    assert ws is big
    assert all(torch.equal(p, q) for p, q in zip(fresh, poisoned))
    assert all(torch.equal(p, q) for p, q in zip(fresh, reused))


def test_stream_kernels_use_no_scratch(kernels):
    meta, _ = kernels
    names = (_find(meta, "greedy_stream_proj_kernel") + _find(meta, "greedy_stream_feed_kernel")
             + _find(meta, "greedy_stream_begin_kernel") + _find(meta, "enc_reset_kernel"))
    assert len(names) == 4
    for k in names + _find(meta, "enc_step_kernel") + _find(meta, "enc_norm_kernel") + _find(meta, "prednet_kernel"):
        assert int(meta[k]["private_segment_fixed_size"]) == 0, k
        assert int(meta[k].get("vgpr_spill_count", "0")) == 0, k
