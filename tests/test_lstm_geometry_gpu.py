"""The three LSTM engines on the MI355X at the launch geometries the older suites never reach (tests/lstm_geometry.py holds the
cases, tests/test_lstm_geometry.py proves on the CPU which geometry each one reaches): partial last row tiles, frames that are
not 16-byte aligned, widths that really pad (H % 8, P % 4, the stacked f P % 4), TR bound by the LDS clamp, the encoder's
input GEMM over several windows, runs of one and two frames, and the row limit.

References and bars are the older suites' own: stock nn.LSTM in float64 on the CPU for the training layer
(test_lstm_train_gpu), the float64 NumPy restatements for the encoder and the prediction step (test_encoder_stream_gpu,
test_prednet_step_gpu); 1e-4 max(1, max|ref|) for y, out, states and pred_proj, and for the training gradients
max(that, 4 x the error of stock float32 nn.LSTM on the GPU against the same reference) per tensor.  Bitwise tests use
torch.equal.  The packed weight images are read back and compared exactly with the weights rearranged on the CPU: the step
kernels stage zeros past K and store no padded column, so a wrong but finite padding cell shows nowhere else.  Every parity
test prints max|ref|, the error and the bar per tensor (DESIGN.md 8g and the encoder / prediction-step sections hold the
tables)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from rnnt_speech_recognition_amd import _lib, joint as jmod, lstm as lmod
from rnnt_speech_recognition_amd.joint import EncoderStream, PredictionStep
from tests import lstm_geometry as geo
from tests import test_encoder_stream_gpu as en
from tests import test_lstm_train_gpu as lt
from tests import test_prednet_step_gpu as pn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INVALID_VALUE = 2  # include/rnnt.h RNNT_STATUS_INVALID_VALUE


def _eq(full, part, rows):
    """Every output of lt._abi_call: `rows` of the full run against a run of those rows alone."""
    for a, b in zip(full, part):
        assert (a is None and b is None) or torch.equal(a[:, rows], b)


def _gate_image(W, Kpad, ld):
    """The packed gate image of W [4N, K] (torch rows i, f, g, o) in float32 on the CPU: [Kpad, ld], column 32 tile + 8 gate + u
    holds unit 8 tile + u of that gate; zeros past N and past K."""
    W = W.detach().cpu()
    N, K = W.shape[0] // 4, W.shape[1]
    c = torch.arange(ld)
    j = (c >> 5) * 8 + (c & 7)
    row, live = ((c >> 3) & 3) * N + j, j < N
    img = torch.zeros(Kpad, ld)
    img[:K, live] = W[row[live]].t()
    return img, live


def _plain_image(W, Kpad, ld):
    """W [K, N] as stored, zero-padded to [Kpad, ld]."""
    W = W.detach().cpu()
    img = torch.zeros(Kpad, ld)
    img[: W.shape[0], : W.shape[1]] = W
    return img


def _image_at(ws, where):
    off, Kpad, ld = where
    return ws.view(torch.float32)[off: off + Kpad * ld].view(Kpad, ld).cpu()


# ---------------------------------------------------------------------------------------------
# the training layer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,R", [(k, R) for k, c in geo.TRAIN.items() for R in c["rows"]])
def test_training_parity_with_float64_lstm(key, R):
    c = geo.TRAIN[key]
    I, H, P, T = c["I"], c["H"], c["P"], c["T"]
    m = lt._layer(I, H, P)
    g = torch.Generator().manual_seed(R + T)
    x, dy = torch.randn(R, T, I, generator=g), torch.randn(R, T, P, generator=g)
    ref = lt._run_module(copy.deepcopy(m).double(), x.double(), dy.double())
    mg = copy.deepcopy(m).to(DEV)
    base = lt._run_module(mg, x.to(DEV), dy.to(DEV))   # stock nn.LSTM, float32, GPU
    got = lt._run_engine(mg, x.to(DEV), dy.to(DEV))
    torch.cuda.synchronize()
    assert len(ref) == len(base) == len(got) == (7 if P < H else 6)
    bad = []
    for name, r, b, e in zip(lt.NAMES, ref, base, got):
        eb, ee = (b - r).abs().max().item(), (e - r).abs().max().item()
        bar = lt._bar(r) if name == "y" else max(lt._bar(r), 4 * eb)
        print(f"lstm_train parity {key} I/H/P={I}/{H}/{P} T={T} R={R} {name}: max|ref|={r.abs().max().item():.3e} "
              f"torch_f32_err={eb:.3e} engine_err={ee:.3e} bar={bar:.3e} branch={'1e-4' if bar == lt._bar(r) else '4x'}")
        assert torch.isfinite(e).all(), name
        if not ee <= bar:
            bad.append((name, ee, bar))
    assert not bad, bad


def _abi_inputs(c, R, T, seed):
    m = lt._layer(c["I"], c["H"], c["P"], seed=seed).to(DEV)
    g = torch.Generator().manual_seed(seed + 4)
    return m, torch.randn(T, R, 4 * c["H"], generator=g).to(DEV), torch.randn(T, R, c["P"], generator=g).to(DEV)


@pytest.mark.parametrize("key", ["ragged_proj", "ragged_unproj"])
def test_training_rows_are_bitwise_independent_of_the_row_tiles(key):
    c = geo.TRAIN[key]
    R = c["rows"][0]
    m, pre, dy = _abi_inputs(c, R, c["T"], seed=1)
    full = lt._abi_call(m, pre, dy)
    for t in full:
        assert t is None or torch.isfinite(t).all()
    for k in geo.TRAIN_ROWS:  # TR = 1 in every role
        _eq(full, lt._abi_call(m, pre[:, k:k + 1].contiguous(), dy[:, k:k + 1].contiguous()), slice(k, k + 1))
    for k in (0, 16, R - 16):  # a block of 16: other TRs again, whole tiles; the last block holds rows 299 and 300
        _eq(full, lt._abi_call(m, pre[:, k:k + 16].contiguous(), dy[:, k:k + 16].contiguous()), slice(k, k + 16))


@pytest.mark.parametrize("key", ["ragged_proj", "ragged_unproj"])
def test_training_poisoned_buffers_at_padded_widths(key, monkeypatch):
    m, pre, dy = _abi_inputs(geo.TRAIN[key], 5, 4, seed=2)
    clean = lt._abi_call(m, pre, dy)
    monkeypatch.setattr(lmod, "_BUFFER_FILL", 0xFF)  # NaN in every float word of the workspace and of the output buffers
    poisoned = lt._abi_call(m, pre, dy)
    monkeypatch.setattr(lmod, "_BUFFER_FILL", None)
    for a, b in zip(clean, poisoned):
        assert (a is None and b is None) or (torch.isfinite(b).all() and torch.equal(a, b))


@pytest.mark.parametrize("key", ["ragged_proj", "ragged_unproj"])
def test_training_weight_images_are_exact_and_zero_padded(key, monkeypatch):
    """"Padding is zeros": the packed images in a poisoned workspace equal the weights rearranged on the CPU, bit for bit,
    with zeros in every padded row and column (an unwritten cell would still hold the poison's NaN)."""
    c = geo.TRAIN[key]
    m, pre, dy = _abi_inputs(c, 5, 2, seed=6)
    kept, real = [], lmod._workspace
    monkeypatch.setattr(lmod, "_workspace", lambda *a: kept.append(real(*a)) or kept[-1])
    monkeypatch.setattr(lmod, "_BUFFER_FILL", 0xFF)
    lt._abi_call(m, pre, dy)
    monkeypatch.setattr(lmod, "_BUFFER_FILL", None)
    assert len(kept) == 2  # the forward's workspace, the backward's
    where, nbytes = geo.lt_images(c["H"], c["P"], 5)
    assert kept[0].numel() == kept[1].numel() == nbytes
    proj = c["P"] < c["H"]
    want = {"whh_f": (kept[0], _gate_image(m.weight_hh_l0, *where["whh_f"][1:])[0]),
            "whh_b": (kept[1], _plain_image(m.weight_hh_l0, *where["whh_b"][1:]))}
    if proj:
        want["whr_f"] = (kept[0], _plain_image(m.weight_hr_l0.t(), *where["whr_f"][1:]))
        want["whr_b"] = (kept[1], _plain_image(m.weight_hr_l0, *where["whr_b"][1:]))
    assert sorted(want) == sorted(where)
    for name, (ws, img) in want.items():
        got = _image_at(ws, where[name])
        assert img.numel() > m.weight_hh_l0.numel() if "hh" in name else img.numel() > m.weight_hr_l0.numel()  # (padding exists)
        assert torch.equal(got, img), (name, int((got != img).sum()))


def test_training_row_limit():
    c = geo.TRAIN["max_rows"]
    R = c["rows"][0]
    assert R == lmod.MAX_ROWS
    m, pre, dy = _abi_inputs(c, R, c["T"], seed=3)
    full = lt._abi_call(m, pre, dy)
    _eq(full, lt._abi_call(m, pre[:, :16].contiguous(), dy[:, :16].contiguous()), slice(0, 16))
    _eq(full, lt._abi_call(m, pre[:, R - 16:].contiguous(), dy[:, R - 16:].contiguous()), slice(R - 16, R))
    over = torch.zeros(c["T"], R + 1, 4 * c["H"], device=DEV)
    with pytest.raises(ValueError):
        lmod.engine_forward(over, m.weight_hh_l0.detach().contiguous(), m.weight_hr_l0.detach().contiguous())
    n = ctypes.c_size_t(0)
    lib = _lib.load()
    assert lib.get_rnnt_lstm_train_workspace_size(R, c["T"], c["H"], c["P"], ctypes.byref(n)) == 0 and n.value > 0
    assert lib.get_rnnt_lstm_train_workspace_size(R + 1, c["T"], c["H"], c["P"], ctypes.byref(n)) == INVALID_VALUE


# ---------------------------------------------------------------------------------------------
# the encoder
# ---------------------------------------------------------------------------------------------
def _report(tag, name, got, want):
    got = got.double().cpu().numpy()
    err, top = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"{tag} {name}: max|ref|={top:.3e} engine_err={err:.3e} bar={1e-4 * max(1.0, top):.3e}")
    assert np.isfinite(got).all(), name


def _encoder_input(c, R, seed):
    enc = en._encoder(*geo.encoder_args(c), seed=seed)
    torch.manual_seed(100 + seed)
    return enc, torch.randn(R, c["T"], c["feat"][0] * c["feat"][1], device=DEV)


def _check_encoder(tag, enc, got, x):
    """got = (out, states, ...) of en._run for the rows x, against the float64 restatement of those rows."""
    want, states = en._restate(enc, x)
    assert tuple(got[0].shape) == want.shape
    _report(tag, "out", got[0], want)
    en._close(got[0], want)
    for i, ((r, c), (rr, cr)) in enumerate(zip(got[1], states)):
        _report(tag, f"r{i}", r, rr)
        _report(tag, f"c{i}", c, cr)
        en._close(r, rr)
        en._close(c, cr)


@pytest.mark.parametrize("name,R", [(k, R) for k, c in geo.ENCODER.items() if k != "windows" for R in c["rows"]])
def test_encoder_run_matches_a_float64_restatement(name, R):
    c = geo.ENCODER[name]
    enc, x = _encoder_input(c, R, seed=R)
    assert EncoderStream(enc).engine
    _check_encoder(f"encoder parity {name} H/P={c['H']}/{c['P']} L={c['L']} f={c['f']} T={c['T']} R={R}", enc, en._run(enc, x), x)


@pytest.mark.parametrize("name,R,rows", [("ragged", 37, (0, 15, 16, 32, 36)), ("lds_tile", 24, (0, 7, 8, 15, 16, 23))])
def test_encoder_rows_are_bitwise_independent_of_the_row_tiles(name, R, rows):
    enc, x = _encoder_input(geo.ENCODER[name], R, seed=5)
    full = en._run(enc, x)
    assert en._same(full, en._run(enc, x))
    for row in rows:
        alone = en._run(enc, x[row: row + 1])
        assert torch.equal(alone[0][0], full[0][row]), row
        assert all(torch.equal(r[0], rf[row]) and torch.equal(c[0], cf[row]) for (r, c), (rf, cf) in zip(alone[1], full[1])), row


@pytest.mark.parametrize("name", ["ragged", "ragged_unproj"])
def test_encoder_poisoned_workspace_at_padded_widths(name, monkeypatch):
    c = geo.ENCODER[name]
    enc, x = _encoder_input(c, c["rows"][0], seed=9)
    cut = [c["f"]]
    fresh = en._run(enc, x, cut)
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", 0xFF)  # NaN in every float word of the workspace before begin
    poisoned = en._run(enc, x, cut)
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", None)
    assert torch.isfinite(poisoned[0]).all() and all(torch.isfinite(r).all() and torch.isfinite(s).all() for r, s in poisoned[1])
    assert en._same(fresh, poisoned)


@pytest.mark.parametrize("name", ["ragged", "ragged_unproj"])
def test_encoder_weight_images_are_exact_and_zero_padded(name, monkeypatch):
    """As for the training layer: W_ih, W_hh, the summed bias and W_hr of every block as begin packs them into a poisoned
    workspace, against the same rearrangement on the CPU, bit for bit, zeros in the padding."""
    c = geo.ENCODER[name]
    R, T = c["rows"][0], c["T"]
    enc = en._encoder(*geo.encoder_args(c), seed=4)
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", 0xFF)
    es = EncoderStream(enc)
    es.begin(R, T)
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", None)
    assert es._use_engine
    torch.cuda.synchronize()
    where, nbytes = geo.en_images(*geo.encoder_args(c), R, T)
    assert es._ws.numel() == nbytes
    for l, (blk, at) in enumerate(zip(enc.blocks, where)):
        lstm = blk.lstm
        want = {"wi": _gate_image(lstm.weight_ih_l0, *at["wi"][1:])[0], "wh": _gate_image(lstm.weight_hh_l0, *at["wh"][1:])[0]}
        bias, live = _gate_image((lstm.bias_ih_l0 + lstm.bias_hh_l0)[:, None], *at["b"][1:])
        want["b"] = bias
        assert (~live).sum() == 4 * (geo.r8(c["H"]) - c["H"]) > 0  # dead units in the last gate tile
        if lstm.proj_size:
            want["wr"] = _plain_image(lstm.weight_hr_l0.t(), *at["wr"][1:])
        assert sorted(want) == sorted(at)
        for key, img in want.items():
            got = _image_at(es._ws, at[key])
            assert torch.equal(got, img), (l, key, int((got != img).sum()))


@pytest.fixture(scope="module")
def windows():
    """The "windows" case, run once: (encoder, x [1024, 37, 12], its single run)."""
    c = geo.ENCODER["windows"]
    enc, x = _encoder_input(c, c["rows"][0], seed=7)
    assert EncoderStream(enc).engine
    return c, enc, x, en._run(enc, x)


def test_encoder_windows_match_a_float64_restatement(windows):
    c, enc, x, full = windows
    rows = torch.tensor(geo.WINDOW_ROWS, device=DEV)
    got = (full[0][rows], [(r[rows], s[rows]) for r, s in full[1]])
    _check_encoder(f"encoder parity windows H/P={c['H']}/{c['P']} L={c['L']} f={c['f']} T={c['T']} R={x.shape[0]} rows={geo.WINDOW_ROWS}",
                   enc, got, x[rows])


def test_encoder_windows_rows_equal_one_window_runs(windows):
    c, enc, x, full = windows
    R = x.shape[0]
    for a in (0, R - 16):  # R = 16: the whole run fits in one window
        part = en._run(enc, x[a: a + 16])
        assert torch.equal(part[0], full[0][a: a + 16]), a
        for (r, s), (rf, sf) in zip(part[1], full[1]):
            assert torch.equal(r, rf[a: a + 16]) and torch.equal(s, sf[a: a + 16]), a


def test_encoder_windows_chunks_equal_the_single_run(windows):
    c, enc, x, full = windows
    f, T = c["f"], c["T"]
    assert 16 % f == 0 and 20 % f == 0
    # cuts at a window boundary, inside a window, and before the odd tail: every chunk is at most one window long
    assert en._same(full, en._run(enc, x, [16, 20, f * (T // f)]))


def test_encoder_row_limit():
    c = geo.ENCODER["short_T1"]
    enc = en._encoder(*geo.encoder_args(c), seed=1)
    es = EncoderStream(enc)
    es.begin(4, 4)
    assert es._use_engine
    lib, n = _lib.load(), ctypes.c_size_t(0)
    args = (es._blocks, len(es._blocks), es.F, es.ridx, es.factor)
    assert lib.get_rnnt_encoder_workspace_size(*args, 1024, 4, ctypes.byref(n)) == 0 and n.value > 0
    assert lib.get_rnnt_encoder_workspace_size(*args, 1025, 4, ctypes.byref(n)) == INVALID_VALUE
    with pytest.raises(RuntimeError):
        _lib.encoder_workspace_bytes(es._blocks, es.F, es.ridx, es.factor, 1025, 4)
    es.begin(1025, 4)  # the Python layer keeps such a batch off the engine
    assert not es._use_engine


# ---------------------------------------------------------------------------------------------
# the prediction step
# ---------------------------------------------------------------------------------------------
def _pred_sequence(R, steps, seed, parents):
    rng = np.random.default_rng(seed)
    seq = []
    for i in range(steps):
        emitted = rng.integers(0, pn.VOCAB, R)
        emitted[rng.random(R) < 0.3] = -1
        seq.append((emitted, rng.integers(0, R, R) if parents and i else None))
    return seq


@pytest.mark.parametrize("name,R", [(k, R) for k, c in geo.PREDNET.items() for R in c["rows"]])
def test_prediction_step_matches_a_float64_restatement(name, R):
    c = geo.PREDNET[name]
    net, W1 = pn._net(*geo.prednet_args(c))
    ps = PredictionStep(net, W1)
    assert ps.engine
    ref = pn._Ref(net, W1, R)
    tag = f"prednet parity {name} E/H/P/J={c['E']}/{c['H']}/{c['P']}/{c['J']} R={R}"
    pp = ps.begin(R)
    _report(tag + " begin", "pred_proj", pp, ref.pp)
    pn._close(pp, ref.pp)
    for i, (emitted, parents) in enumerate(_pred_sequence(R, 3, R, parents=True)):  # three steps: both state slots are read
        pp = ps.step(torch.tensor(emitted, dtype=torch.int32, device=DEV),
                     None if parents is None else torch.tensor(parents, dtype=torch.int32, device=DEV))
        want = ref.step(emitted, parents)
        _report(f"{tag} step{i}", "pred_proj", pp, want)
        pn._close(pp, want)
        assert (pp[:, c["J"]:] == 0).all()
        for l, ((r, s), (rr, sr)) in enumerate(zip(ps.state(), ref.state)):
            _report(f"{tag} step{i}", f"r{l}", r, rr)
            _report(f"{tag} step{i}", f"c{l}", s, sr)
            pn._close(r, rr)
            pn._close(s, sr)


def _pred_run(net, W1, seq, rows):
    ps = PredictionStep(net, W1)
    outs = [ps.begin(len(rows)).clone()]
    for emitted, _ in seq:
        outs.append(ps.step(torch.tensor(emitted[rows], dtype=torch.int32, device=DEV)).clone())
    return outs, [(r.clone(), s.clone()) for r, s in ps.state()]


@pytest.mark.parametrize("name", sorted(geo.PREDNET))
def test_prediction_step_rows_are_bitwise_independent_of_the_row_tiles(name):
    c = geo.PREDNET[name]
    net, W1 = pn._net(*geo.prednet_args(c), seed=3)
    seq = _pred_sequence(37, 3, 2, parents=False)
    full, st = _pred_run(net, W1, seq, np.arange(37))
    rows = np.array([0, 15, 16, 32, 36])  # R = 5: gates TR 8 (16 at R = 37); one row in the dense launches' last tile in both
    part, stp = _pred_run(net, W1, seq, rows)
    for a, b in zip(full, part):
        assert torch.isfinite(a).all() and torch.equal(a[rows], b)
    for (r, s), (rp, sp) in zip(st, stp):
        assert torch.equal(r[rows], rp) and torch.equal(s[rows], sp)


@pytest.mark.parametrize("name", sorted(geo.PREDNET))
def test_prediction_step_poisoned_workspace_at_padded_widths(name, monkeypatch):
    c = geo.PREDNET[name]
    net, W1 = pn._net(*geo.prednet_args(c), seed=4)
    seq = _pred_sequence(5, 3, 9, parents=False)
    fresh = _pred_run(net, W1, seq, np.arange(5))
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", 0xFF)  # NaN in every float word of the workspace before begin
    poisoned = _pred_run(net, W1, seq, np.arange(5))
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", None)
    for a, b in zip(fresh[0], poisoned[0]):
        assert torch.isfinite(b).all() and torch.equal(a, b)
    for (r, s), (rp, sp) in zip(fresh[1], poisoned[1]):
        assert torch.isfinite(rp).all() and torch.isfinite(sp).all() and torch.equal(r, rp) and torch.equal(s, sp)


def test_prediction_step_row_limit():
    c = geo.PREDNET["ragged_proj"]
    net, W1 = pn._net(*geo.prednet_args(c))
    ps = PredictionStep(net, W1)
    ps.begin(4)
    assert ps._use_engine
    lib, n = _lib.load(), ctypes.c_size_t(0)
    args = (ps._blocks, len(ps._blocks), ps.E, ps.V, ps.Jp)
    assert lib.get_rnnt_prednet_workspace_size(*args, 1024, ctypes.byref(n)) == 0 and n.value > 0
    assert lib.get_rnnt_prednet_workspace_size(*args, 1025, ctypes.byref(n)) == INVALID_VALUE
    with pytest.raises(RuntimeError):
        _lib.prednet_workspace_bytes(ps._blocks, ps.E, ps.V, ps.Jp, 1025)
    ps.begin(1025)  # the Python layer keeps such a batch off the engine
    assert not ps._use_engine
