"""CPU tests of the LSTM layer for training (lstm.LSTMLayerFunction, model.Transducer(lstm=...), the C ABI's argument checks and
the code object of the new step kernels).  The reference for every comparison is stock torch.nn.LSTM in float64 on the CPU with
the same weights, inputs and dy, through torch's own autograd.  Both sides are float64, so the bar 1e-10 max(1, max|ref|) only
allows for summation order: a failure here is a wrong formula, not rounding."""
import ctypes
import os

import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib, lstm as lmod, train
from rnnt_speech_recognition_amd.lstm import LSTMLayerFunction
from tests.test_isa_audit import READELF, OBJDUMP, _find, kernels  # noqa: F401  (module-scoped fixture: the built code objects)


def _close(got, ref, what):
    err = (got - ref).abs().max().item() if ref.numel() else 0.0
    assert err <= 1e-10 * max(1.0, ref.abs().max().item() if ref.numel() else 0.0), (what, err)


# (I, H, P): projected, unprojected, odd widths
WIDTHS = [(12, 32, 16), (12, 24, 24), (12, 20, 9)]


@pytest.mark.parametrize("I,H,P", WIDTHS)
@pytest.mark.parametrize("T", [1, 2, 37])
@pytest.mark.parametrize("R", [1, 5])
def test_equations_reproduce_nn_lstm_in_float64(I, H, P, T, R):
    torch.manual_seed(100 * T + R)
    ref = torch.nn.LSTM(I, H, proj_size=P if P < H else 0, batch_first=True).double()
    x = torch.randn(R, T, I, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(R, T, P, dtype=torch.float64)
    y, _ = ref(x)
    y.backward(dy)
    want = {"x": x.grad.clone(), **{k: p.grad.clone() for k, p in ref.named_parameters()}}
    x.grad = None
    ref.zero_grad()
    y2 = lmod.lstm_layer(ref, x)
    assert y2.shape == y.shape and y2.dtype == torch.float64
    y2.backward(dy)
    _close(y2.detach(), y.detach(), "y")
    _close(x.grad, want["x"], "dx")
    for k, p in ref.named_parameters():
        _close(p.grad, want[k], k)
    # the bias gradient goes to both vectors, and dW_hh is the one-frame shift (zero for a single frame)
    assert torch.equal(ref.bias_ih_l0.grad, ref.bias_hh_l0.grad)
    if T == 1:
        assert not ref.weight_hh_l0.grad.any()


def test_gradients_accumulate_and_unneeded_ones_are_skipped():
    torch.manual_seed(0)
    m = torch.nn.LSTM(6, 10, proj_size=4, batch_first=True).double()
    x = torch.randn(3, 5, 6, dtype=torch.float64)  # no gradient wanted: the encoder's first layer
    lmod.lstm_layer(m, x).sum().backward()
    first = {k: p.grad.clone() for k, p in m.named_parameters()}
    assert x.grad is None
    lmod.lstm_layer(m, x).sum().backward()
    for k, p in m.named_parameters():
        _close(p.grad, 2 * first[k], k)
    m.weight_ih_l0.requires_grad_(False)
    m.zero_grad()
    m.weight_ih_l0.grad = None
    lmod.lstm_layer(m, x).sum().backward()
    assert m.weight_ih_l0.grad is None
    _close(m.weight_hh_l0.grad, first["weight_hh_l0"], "weight_hh_l0")


def test_double_backward_raises():
    torch.manual_seed(0)
    m = torch.nn.LSTM(6, 10, batch_first=True).double()
    x = torch.randn(2, 4, 6, dtype=torch.float64, requires_grad=True)
    (gx,) = torch.autograd.grad(lmod.lstm_layer(m, x).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def test_unknown_route_raises():
    hp = _small_hp()
    with pytest.raises(ValueError):
        pkg.Transducer(hp, lstm="cudnn")
    with pytest.raises(ValueError):
        pkg.Encoder(hp, lstm="")
    with pytest.raises(ValueError):
        pkg.PredictionNetwork(hp, lstm=None)
    with pytest.raises(ValueError):
        pkg.model._LSTMBlock(4, 8, 4, 0.0, lstm="Engine")


def _small_hp():
    # a projected encoder (24 / 16) with the reduction in the middle, an unprojected prediction network (16 / 16)
    return pkg.HParams(vocab_size=11, mel_bins=4, downsample_factor=3, embedding_size=7, encoder_layers=3, encoder_size=24,
                       projection_size=16, time_reduction_index=1, time_reduction_factor=2, pred_net_layers=2, pred_net_size=16,
                       joint_net_size=12)


def _pair(dtype=torch.float64):
    hp = _small_hp()
    torch.manual_seed(7)
    a = pkg.Transducer(hp, lstm="torch")
    torch.manual_seed(7)
    b = pkg.Transducer(hp, lstm="engine")
    return hp, a.to(dtype), b.to(dtype)


def test_routes_share_parameters_and_checkpoints(tmp_path):
    hp, a, b = _pair(torch.float32)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys())
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert pkg.Transducer(hp).lstm_route == "torch" and b.lstm_route == "engine"
    assert all(blk.lstm_route == "engine" for blk in list(b.encoder.blocks) + list(b.prediction.blocks))
    with torch.no_grad():
        for p in a.parameters():
            p.add_(0.25)
    pkg.model.save_weights(a, str(tmp_path / "a.pt"))
    pkg.model.load_weights(b, str(tmp_path / "a.pt"))
    for k, v in b.state_dict().items():
        assert torch.equal(v, a.state_dict()[k]), k
    pkg.model.save_weights(b, str(tmp_path / "b.pt"))
    c = pkg.Transducer(hp, lstm="torch")
    pkg.model.load_weights(c, str(tmp_path / "b.pt"))
    for k, v in c.state_dict().items():
        assert torch.equal(v, a.state_dict()[k]), k
    # the initialisers act on the nn.LSTM the block holds, whatever the route
    pkg.model.init_lstm_like_tf1_(b.encoder.blocks[0].lstm)
    assert b.encoder.blocks[0].lstm.bias_ih_l0[24:48].eq(1).all()


def test_routes_agree_on_outputs_and_every_gradient_in_float64():
    hp, a, b = _pair()
    mel, pred_inp, _, _, _ = train.synthetic_batch(hp, 3, 21, 6, "cpu", seed=5)
    a.train(), b.train()
    grads = {}
    outs = {}
    for name, m in (("torch", a), ("engine", b)):
        m.zero_grad()
        enc, pred = m(mel.double(), pred_inp)
        (enc.sum() + (pred * pred).sum() + (enc * enc).sum()).backward()  # (the fused joint needs a GPU)
        outs[name] = (enc.detach(), pred.detach())
        grads[name] = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    _close(outs["engine"][0], outs["torch"][0], "enc")
    _close(outs["engine"][1], outs["torch"][1], "pred")
    assert grads["torch"].keys() == grads["engine"].keys() and len(grads["torch"]) >= 20
    for k, g in grads["torch"].items():
        assert g.abs().max() > 0, k
        _close(grads["engine"][k], g, k)


def test_train_step_takes_an_engine_model_on_the_cpu_up_to_the_joint():
    hp, _, b = _pair(torch.float32)
    step = pkg.TrainStep(b, global_batch=2)
    assert len(step.params) == len(list(b.parameters()))


def test_cuda_only_helpers_refuse_cpu_tensors():
    pre = torch.zeros(2, 1, 16)
    with pytest.raises(TypeError):
        lmod.engine_forward(pre, torch.zeros(16, 4), None)
    with pytest.raises(TypeError):
        lmod.engine_backward(pre, torch.zeros(2, 1, 4), torch.zeros(2, 1, 4), torch.zeros(16, 4), None)


def test_symbols_are_declared_and_exported():
    names = ["get_rnnt_lstm_train_workspace_size", "compute_rnnt_lstm_train_fwd", "compute_rnnt_lstm_train_bwd"]
    pkg.build()
    lib = _lib.load()
    for n in names:
        assert n in _lib.SYMBOLS
        assert ctypes.cast(getattr(lib, n), ctypes.c_void_p).value
    assert pkg.LSTMLayerFunction is LSTMLayerFunction


def test_argument_validation_needs_no_device():
    pkg.build()
    lib = _lib.load()
    n = ctypes.c_size_t(0)
    assert lib.get_rnnt_lstm_train_workspace_size(64, 600, 320, 320, ctypes.byref(n)) == 0
    unproj = n.value
    assert unproj % 256 == 0 and unproj >= 4 * (2 * 320 * 1280 + 64 * 320)
    assert lib.get_rnnt_lstm_train_workspace_size(64, 600, 2048, 640, ctypes.byref(n)) == 0
    assert n.value >= 4 * 2 * (640 * 8192 + 2048 * 640)
    assert _lib.lstm_train_workspace_bytes(64, 600, 320, 320) == unproj
    for bad in ((0, 600, 320, 320), (64, 0, 320, 320), (64, 600, 0, 320), (64, 600, 320, 0), (-1, 600, 320, 320),
                (64, 600, 320, 321), (1025, 600, 320, 320), (64, 600, 4097, 640)):
        assert lib.get_rnnt_lstm_train_workspace_size(*bad, ctypes.byref(n)) == 2, bad
    assert lib.get_rnnt_lstm_train_workspace_size(64, 600, 320, 320, None) == 2

    fake = ctypes.c_void_p(256)  # never dereferenced: rejected before any launch
    o = _lib.make_options(0, 0, 1, 1)

    def fwd(gates=fake, w_hh=fake, w_hr=None, y=fake, c=fake, h=None, R=4, T=3, H=32, P=32, ws=fake, opts=o):
        return lib.compute_rnnt_lstm_train_fwd(gates, w_hh, w_hr, y, c, h, R, T, H, P, ws, opts)

    def bwd(gates=fake, c=fake, dy=fake, w_hh=fake, w_hr=None, dr=None, R=4, T=3, H=32, P=32, ws=fake, opts=o):
        return lib.compute_rnnt_lstm_train_bwd(gates, c, dy, w_hh, w_hr, dr, R, T, H, P, ws, opts)

    for call in (fwd, bwd):
        for kw in (dict(R=0), dict(T=0), dict(H=0), dict(P=0), dict(R=-3), dict(P=33), dict(P=16),  # P < H without W_hr
                   dict(w_hr=fake), dict(w_hr=fake, P=32),                                          # W_hr with P = H
                   dict(gates=None), dict(w_hh=None), dict(c=None), dict(ws=None), dict(ws=ctypes.c_void_p(260)),
                   dict(gates=ctypes.c_void_p(260)), dict(opts=_lib.make_options(0, 0, 1, 1, loc=_lib.RNNT_CPU))):
            assert call(**kw) == 2, (call.__name__, kw)
    assert fwd(y=None) == 2 and bwd(dy=None) == 2
    assert fwd(w_hr=fake, P=16, h=None) == 2      # a projected layer needs h
    assert bwd(w_hr=fake, P=16, dr=None) == 2     # ... and dr
    if not torch.cuda.is_available():  # with a device a valid call would enqueue on the fake pointers
        assert fwd() != 2 and bwd() != 2
        assert fwd(w_hr=fake, P=16, h=fake) != 2 and bwd(w_hr=fake, P=16, dr=fake) != 2


@pytest.mark.skipif(not (os.path.exists(READELF) and os.path.exists(OBJDUMP)), reason="ROCm LLVM tools absent")
def test_step_kernels_use_no_scratch_and_do_not_spill(kernels):  # noqa: F811
    meta, _ = kernels
    step = _find(meta, "lstm_train_step_kernel")
    # four roles x rows per workgroup {1, 2, 4, 8, 16} x k groups {32, 64}
    assert len(step) == 40
    for k in step + _find(meta, "lstm_train_pack_kernel"):
        m = meta[k]
        assert int(m["private_segment_fixed_size"]) == 0, (k, m["private_segment_fixed_size"])
        assert int(m.get("vgpr_spill_count", "0")) == 0 and int(m.get("sgpr_spill_count", "0")) == 0, k
        assert int(m["vgpr_count"]) <= 128, (k, m["vgpr_count"])  # 512 threads: two workgroups of 8 waves fit a CU's registers
