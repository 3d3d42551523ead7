"""The prediction-network step (joint.PredictionStep, include/rnnt.h compute_rnnt_prednet_*), CPU side: the torch route's state
machine against the composition the decoders used before it, the decoders' prediction="engine" route against the default one,
and the C ABI's argument checks (no device needed)."""
import ctypes

import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib, decoding
from rnnt_speech_recognition_amd.joint import PredictionStep
from tests.test_frontend import small_model


def _model(seed=0, vocab=12, layers=1):
    torch.manual_seed(seed)
    hp = pkg.HParams(vocab_size=vocab, mel_bins=4, downsample_factor=2, embedding_size=8, encoder_layers=2, encoder_size=16,
                     projection_size=8, time_reduction_index=0, pred_net_layers=layers, pred_net_size=16, joint_net_size=64)
    return pkg.Transducer(hp).eval()


@pytest.mark.parametrize("layers,beam", [(1, False), (2, False), (2, True)])
def test_prediction_step_matches_the_torch_composition(layers, beam):
    model = _model(1, layers=layers)
    net, W1 = model.prediction, model.joint.W1.detach()
    R = 6
    gen = torch.Generator().manual_seed(7)
    ps = PredictionStep(net, W1)
    assert not ps.engine
    pp = ps.begin(R)
    with torch.no_grad():
        g, states = decoding._pred_step(net, torch.zeros(R, dtype=torch.int32), [None] * layers)
        assert torch.equal(pp, g @ W1)
        for _ in range(20):
            emitted = torch.randint(0, 12, (R,), generator=gen, dtype=torch.int32)
            emitted[torch.rand(R, generator=gen) < 0.4] = -1
            parents = torch.randint(0, R, (R,), generator=gen, dtype=torch.int32) if beam else None
            pp = ps.step(emitted, parents)
            if parents is not None:
                idx = parents.long()
                g, states = g[idx], [(h[:, idx], c[:, idx]) for h, c in states]
            mask = emitted >= 0
            g2, st2 = decoding._pred_step(net, emitted.clamp(min=0), states)
            g = torch.where(mask[:, None], g2, g)
            states = [(torch.where(mask[None, :, None], h2, h), torch.where(mask[None, :, None], c2, c))
                      for (h2, c2), (h, c) in zip(st2, states)]
            assert torch.equal(pp, g @ W1)
            for (r, c), (h_ref, c_ref) in zip(ps.state(), states):
                assert torch.equal(r, h_ref[0]) and torch.equal(c, c_ref[0])


@pytest.mark.parametrize("cap", [None, 1])
def test_engine_prediction_route_decodes_like_the_torch_route_greedy(cap):
    model = small_model(3)
    torch.manual_seed(4)
    mel = torch.randn(5, 24, 8)
    sl = torch.tensor([24, 11, 24, 6, 17])
    a = decoding.greedy_decode_batch(model, mel, sl, max_length=30, max_symbols_per_frame=cap)
    b = decoding.greedy_decode_batch(model, mel, sl, max_length=30, max_symbols_per_frame=cap, prediction="engine")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    torch.testing.assert_close(a[2], b[2], rtol=1e-5, atol=1e-5)
    fa = decoding.greedy_decode_batch_fn(model)(mel, 30, sl)
    fb = decoding.greedy_decode_batch_fn(model, prediction="engine")(mel, 30, sl)
    assert torch.equal(fa[0], fb[0])


@pytest.mark.parametrize("K", [1, 3])
def test_engine_prediction_route_decodes_like_the_torch_route_beam(K):
    model = small_model(3)
    torch.manual_seed(5)
    mel = torch.randn(4, 20, 8)
    sl = torch.tensor([20, 9, 20, 13])
    a = decoding.beam_decode_batch(model, mel, sl, beam=K)
    b = decoding.beam_decode_batch(model, mel, sl, beam=K, prediction="engine")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    torch.testing.assert_close(a[2], b[2], rtol=1e-5, atol=1e-5)
    fa = decoding.beam_decode_batch_fn(model, beam=K)(mel, None, sl)
    fb = decoding.beam_decode_batch_fn(model, beam=K, prediction="engine")(mel, None, sl)
    assert torch.equal(fa[0], fb[0])


def test_prediction_keyword_is_checked():
    model = small_model(3)
    with pytest.raises(ValueError):
        decoding.greedy_decode_batch(model, torch.randn(1, 6, 8), prediction="tf")
    with pytest.raises(ValueError):
        decoding.beam_decode_batch_fn(model, prediction="cuda")


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    pkg.build()
    return _lib.load()


def _blocks(n=2, H=256, P=128, fake=256):
    arr = (_lib.rnntPrednetBlock * n)()
    for b in arr:
        b.W_ih = b.W_hh = b.b_ih = b.b_hh = b.W_hr = b.ln_weight = b.ln_bias = fake
        b.hidden, b.proj, b.ln_eps = H, P, 1e-3
    return arr


def test_prednet_argument_validation_needs_no_device(lib):
    fake = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before any launch
    n = ctypes.c_size_t(0)
    blocks = _blocks()
    assert lib.get_rnnt_prednet_workspace_size(blocks, 2, 64, 4096, 640, 16, ctypes.byref(n)) == 0
    assert n.value > 0 and n.value % 256 == 0
    small = n.value
    assert lib.get_rnnt_prednet_workspace_size(blocks, 2, 64, 4096, 640, 1024, ctypes.byref(n)) == 0 and n.value > small
    assert lib.get_rnnt_prednet_workspace_size(blocks, 2, 64, 4096, 640, 16, None) == 2
    for args in ((None, 2, 64, 4096, 640, 16), (blocks, 0, 64, 4096, 640, 16), (blocks, 9, 64, 4096, 640, 16),
                 (blocks, 2, 0, 4096, 640, 16), (blocks, 2, 4097, 4096, 640, 16), (blocks, 2, 64, 0, 640, 16),
                 (blocks, 2, 64, 4096, 600, 16), (blocks, 2, 64, 4096, 768, 16), (blocks, 2, 64, 4096, 0, 16),
                 (blocks, 2, 64, 4096, 640, 0), (blocks, 2, 64, 4096, 640, 1025)):
        assert lib.get_rnnt_prednet_workspace_size(*args, ctypes.byref(n)) == 2, args
    for bad in (dict(hidden=0), dict(hidden=4097), dict(proj=4097), dict(proj=0), dict(W_hr=None), dict(ln_eps=float("nan"))):
        arr = _blocks()
        for k, v in bad.items():
            setattr(arr[1], k, v)
        assert lib.get_rnnt_prednet_workspace_size(arr, 2, 64, 4096, 640, 16, ctypes.byref(n)) == 2, bad

    o = _lib.make_options(0, 0, 1, 1)

    def begin(emb=fake, blk=blocks, L=2, E=64, V=4096, w1=fake, J=640, R=16, out=fake, ws=fake, opts=o):
        return lib.compute_rnnt_prednet_begin(emb, blk, L, E, V, w1, J, R, out, ws, opts)

    def step(em=fake, pa=None, out=fake, blk=blocks, L=2, E=64, V=4096, J=640, R=16, ws=fake, opts=o):
        return lib.compute_rnnt_prednet_step(em, pa, out, blk, L, E, V, J, R, ws, opts)

    cpu = _lib.make_options(0, 0, 1, 1, loc=_lib.RNNT_CPU)
    mis16, mis256 = ctypes.c_void_p(256 + 4), ctypes.c_void_p(256 + 64)
    for call in (begin, step):
        assert call(opts=cpu) == 2        # device-only library
        assert call(ws=None) == 2
        assert call(ws=mis256) == 2       # workspace not 256-byte aligned
        assert call(out=None) == 2 and call(out=mis16) == 2
        assert call(blk=None) == 2 and call(L=0) == 2 and call(L=9) == 2
        assert call(R=0) == 2 and call(R=1025) == 2
        assert call(J=600) == 2 and call(J=768) == 2
        assert call(E=4097) == 2 and call(V=0) == 2
    assert begin(emb=None) == 2 and begin(emb=mis16) == 2 and begin(w1=None) == 2 and begin(w1=mis16) == 2
    for field in ("W_ih", "W_hh", "b_ih", "b_hh", "ln_weight", "ln_bias"):
        arr = _blocks()
        setattr(arr[0], field, None)
        assert begin(blk=arr) == 2, field
        setattr(arr[0], field, 256 + 4)
        assert begin(blk=arr) == 2, field
    arr = _blocks()
    arr[1].W_hr = 256 + 8
    assert begin(blk=arr) == 2
    assert step(em=None) == 2 and step(em=mis16) == 2 and step(pa=mis16) == 2
