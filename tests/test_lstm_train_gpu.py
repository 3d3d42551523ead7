"""The LSTM layer for training on the MI355X (include/rnnt.h compute_rnnt_lstm_train_fwd / _bwd, lstm.LSTMLayerFunction,
model.Transducer(lstm="engine")): parity of y and of every gradient with stock nn.LSTM in float64 on the CPU, bitwise row
independence of the C ABI's outputs, run-to-run equality, poisoned buffers, a whole train step against the torch route, and
decoding after an engine train step.

The bar.  y: 1e-4 max(1, max|ref|), the project's bar for its exact-f32 paths.  Gradients: stock nn.LSTM in float32 on the GPU
is run on the same inputs and its error against the float64 reference is taken per tensor; the engine's error may be at most
max(1e-4 max(1, max|ref|), 4 x that error).  Both errors are printed per tensor and shape (DESIGN.md 8g holds the table)."""
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import decoding, lstm as lmod, train

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("y", "dx", "dW_ih", "dW_hh", "db_ih", "db_hh", "dW_hr")

# (I, H, P, T, rows): small projected; configs[2]'s layer; odd widths; the reference default layer
SHAPES = {
    "small": (12, 256, 128, 50, (1, 16, 64)),
    "configs2": (240, 320, 320, 600, (64,)),
    "odd": (13, 200, 72, 31, (1, 16, 64)),
    "ref": (640, 2048, 640, 150, (16,)),
}
CASES = [(k, r) for k, v in SHAPES.items() for r in v[4]]


def _layer(I, H, P, seed=0):
    torch.manual_seed(seed)
    m = torch.nn.LSTM(I, H, proj_size=P if P < H else 0, batch_first=True)
    pkg.model.init_lstm_like_tf1_(m)  # glorot weights, forget bias 1
    with torch.no_grad():
        m.bias_ih_l0.add_(torch.randn(4 * H) * 0.1), m.bias_hh_l0.add_(torch.randn(4 * H) * 0.1)
    return m


def _run_module(m, x, dy):
    """nn.LSTM through torch's autograd -> [y, dx, dW_ih, dW_hh, db_ih, db_hh, (dW_hr)] on the CPU in float64."""
    x = x.clone().requires_grad_(True)
    m.zero_grad()
    y, _ = m(x)
    y.backward(dy)
    out = [y.detach(), x.grad] + [m.weight_ih_l0.grad, m.weight_hh_l0.grad, m.bias_ih_l0.grad, m.bias_hh_l0.grad]
    if m.proj_size:
        out.append(m.weight_hr_l0.grad)
    return [t.detach().double().cpu() for t in out]


def _run_engine(m, x, dy):
    x = x.clone().requires_grad_(True)
    m.zero_grad()
    y = lmod.lstm_layer(m, x)
    y.backward(dy)
    out = [y.detach(), x.grad] + [m.weight_ih_l0.grad, m.weight_hh_l0.grad, m.bias_ih_l0.grad, m.bias_hh_l0.grad]
    if m.proj_size:
        out.append(m.weight_hr_l0.grad)
    return [t.detach().double().cpu() for t in out]


def _bar(ref):
    return 1e-4 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("key,R", CASES)
def test_parity_with_float64_lstm(key, R):
    I, H, P, T, _ = SHAPES[key]
    m = _layer(I, H, P)
    g = torch.Generator().manual_seed(R)
    x, dy = torch.randn(R, T, I, generator=g), torch.randn(R, T, P, generator=g)
    import copy

    ref = _run_module(copy.deepcopy(m).double(), x.double(), dy.double())
    mg = copy.deepcopy(m).to(DEV)
    base = _run_module(mg, x.to(DEV), dy.to(DEV))   # stock nn.LSTM, float32, GPU
    got = _run_engine(mg, x.to(DEV), dy.to(DEV))
    torch.cuda.synchronize()
    assert len(ref) == len(base) == len(got)
    bad = []
    for name, r, b, e in zip(NAMES, ref, base, got):
        eb, ee = (b - r).abs().max().item(), (e - r).abs().max().item()
        bar = _bar(r) if name == "y" else max(_bar(r), 4 * eb)
        print(f"lstm_train parity {key} I/H/P={I}/{H}/{P} T={T} R={R} {name}: max|ref|={r.abs().max().item():.3e} "
              f"torch_f32_err={eb:.3e} engine_err={ee:.3e} bar={bar:.3e} branch={'1e-4' if bar == _bar(r) else '4x'}")
        assert torch.isfinite(e).all(), name
        if not ee <= bar:
            bad.append((name, ee, bar))
    assert not bad, bad


def _abi_call(m, pre, dy):
    """The C ABI's outputs for time-major pre [T, R, 4H] and dy [T, R, P]: (y, c, h, gates, da, dr)."""
    w_hh = m.weight_hh_l0.detach().contiguous()
    w_hr = m.weight_hr_l0.detach().contiguous() if m.proj_size else None
    gates = pre.clone()
    y, c, h = lmod.engine_forward(gates, w_hh, w_hr)
    da = gates.clone()
    dr = lmod.engine_backward(da, c, dy.contiguous(), w_hh, w_hr)
    torch.cuda.synchronize()
    return y, c, h, gates, da, dr


@pytest.mark.parametrize("key", ["small", "configs2", "odd"])
def test_rows_are_bitwise_independent_and_calls_repeat(key):
    I, H, P, T, _ = SHAPES[key]
    T = min(T, 40)
    m = _layer(I, H, P, seed=1).to(DEV)
    R = 64
    g = torch.Generator().manual_seed(5)
    pre = torch.randn(T, R, 4 * H, generator=g).to(DEV)
    dy = torch.randn(T, R, P, generator=g).to(DEV)
    full = _abi_call(m, pre, dy)
    again = _abi_call(m, pre, dy)
    for a, b in zip(full, again):
        assert (a is None and b is None) or torch.equal(a, b)
    perm = torch.randperm(R, generator=g).to(DEV)
    permuted = _abi_call(m, pre[:, perm].contiguous(), dy[:, perm].contiguous())
    for a, b in zip(full, permuted):
        assert (a is None and b is None) or torch.equal(a[:, perm], b)
    for k in (0, 17, 63):
        alone = _abi_call(m, pre[:, k:k + 1].contiguous(), dy[:, k:k + 1].contiguous())
        for a, b in zip(full, alone):
            assert (a is None and b is None) or torch.equal(a[:, k:k + 1], b)
    sub = _abi_call(m, pre[:, :16].contiguous(), dy[:, :16].contiguous())  # another row tile
    for a, b in zip(full, sub):
        assert (a is None and b is None) or torch.equal(a[:, :16], b)


@pytest.mark.parametrize("key", ["small", "odd", "configs2"])
def test_poisoned_buffers_change_nothing(key, monkeypatch):
    I, H, P, T, _ = SHAPES[key]
    T = min(T, 20)
    m = _layer(I, H, P, seed=2).to(DEV)
    g = torch.Generator().manual_seed(6)
    pre, dy = torch.randn(T, 16, 4 * H, generator=g).to(DEV), torch.randn(T, 16, P, generator=g).to(DEV)
    clean = _abi_call(m, pre, dy)
    monkeypatch.setattr(lmod, "_BUFFER_FILL", 0xFF)  # NaN in every float word of the workspace and of the output buffers
    poisoned = _abi_call(m, pre, dy)
    monkeypatch.setattr(lmod, "_BUFFER_FILL", None)
    for a, b in zip(clean, poisoned):
        assert (a is None and b is None) or (torch.isfinite(b).all() and torch.equal(a, b))


def _configs2_hp():
    return pkg.HParams(vocab_size=28, embedding_size=320, encoder_layers=2, encoder_size=320, projection_size=320,
                       time_reduction_index=0, pred_net_layers=1, pred_net_size=320, joint_net_size=320)  # bench.py bench_e2e


def _models():
    hp = _configs2_hp()
    torch.manual_seed(3)
    a = pkg.Transducer(hp, lstm="torch")
    torch.manual_seed(3)
    b = pkg.Transducer(hp, lstm="engine")
    return hp, a.to(DEV), b.to(DEV)


class _F64Transducer(torch.nn.Module):
    """The torch route with the encoder and the prediction network in float64, feeding the same fused (float32) joint."""

    def __init__(self, model):
        super().__init__()
        import copy

        self.encoder, self.prediction = copy.deepcopy(model.encoder).double(), copy.deepcopy(model.prediction).double()
        self.joint, self.hp = copy.deepcopy(model.joint), model.hp

    def loss(self, mel, pred_inp, spec_len, lab_len, labels):
        enc, pred = self.encoder(mel.double()).float(), self.prediction(pred_inp).float()
        return self.joint(enc, pred, labels, pkg.reduced_lengths(spec_len, self.hp.time_reduction_factor), lab_len)


def test_whole_train_step_matches_the_torch_route():
    hp, mt, me = _models()
    batch = train.synthetic_batch(hp, 8, 600, 40, DEV, seed=11)
    mt.train(), me.train()
    ref = _F64Transducer(mt).train()
    results = {}
    for name, mdl in (("ref", ref), ("torch", mt), ("engine", me)):
        mdl.zero_grad()
        costs = mdl.loss(*batch)
        costs.sum().backward()
        results[name] = (costs.detach().double().cpu(), {k: p.grad.detach().double().cpu() for k, p in mdl.named_parameters()})
    torch.cuda.synchronize()
    ct, ce = results["torch"][0], results["engine"][0]
    print("lstm_train step costs: torch", ct.tolist(), "engine", ce.tolist())
    assert ((ce - ct).abs() <= 1e-4 * ct.abs()).all()
    bad = []
    for k, r in results["ref"][1].items():
        eb = (results["torch"][1][k] - r).abs().max().item()
        ee = (results["engine"][1][k] - r).abs().max().item()
        bar = max(_bar(r), 4 * eb)
        print(f"lstm_train step grad {k}: max|ref|={r.abs().max().item():.3e} torch_f32_err={eb:.3e} engine_err={ee:.3e} "
              f"bar={bar:.3e} branch={'1e-4' if bar == _bar(r) else '4x'}")
        if not ee <= bar:
            bad.append((k, ee, bar))
    assert not bad, bad
    for name, mdl in (("torch", mt), ("engine", me)):
        step = pkg.TrainStep(mdl, global_batch=8, learning_rate=1e-3)
        losses = [step(*batch)["loss"] for _ in range(10)]
        print(f"lstm_train ten steps, {name}: {losses[0]:.4f} -> {losses[-1]:.4f}")
        assert losses[-1] < losses[0], (name, losses)


def test_decoding_after_an_engine_train_step():
    hp, _, me = _models()
    batch = train.synthetic_batch(hp, 4, 120, 12, DEV, seed=12)
    step = pkg.TrainStep(me, global_batch=4, learning_rate=1e-3)
    step(*batch)
    me.eval()
    mel, _, spec_len = batch[0], batch[1], batch[2]
    ids_t, len_t, _ = decoding.greedy_decode_batch(me, mel, spec_len, max_length=30)
    ids_e, len_e, _ = decoding.greedy_decode_batch(me, mel, spec_len, max_length=30, prediction="engine", encoder="engine")
    assert len_t.tolist() == len_e.tolist()
    n = min(ids_t.shape[1], ids_e.shape[1])
    assert torch.equal(ids_t[:, :n].cpu(), ids_e[:, :n].cpu())


def test_non_float32_cuda_tensor_is_an_error():
    m = _layer(12, 32, 16).to(DEV).double()
    with pytest.raises(TypeError):
        lmod.lstm_layer(m, torch.randn(2, 3, 12, dtype=torch.float64, device=DEV))
