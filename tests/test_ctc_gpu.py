"""GPU tests of the CTC loss and the greedy CTC decoder (include/rnnt_ctc.h) through the C ABI, against the float64 restatement of
tests/ctc_cases.py (torch's float64 CPU CTC for the largest lattices).

Bars: the project's fixed ones -- costs within 1e-4 max(1, |cost|), gradients within 1e-4 |cost_scale| absolute; padded frames are
exact zeros, an utterance without a path costs +inf exactly with exact zeros.  Every call gets a gradient buffer and a workspace
filled with 0xFF bytes (a backward-only call: the workspace its forward left).  The measured maxima are printed and, with
CTC_ACCURACY_DIR set, collected in ctc_accuracy.json in that directory (kept in profiles/ctc_notes.md)."""
import json
import os

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib
from tests import ctc_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTOL = GTOL = 1e-4
CONST = cc.header_constants()


def _record(route, **figures):
    row = {k: float(v) for k, v in figures.items()}
    print(route, row)
    out = os.environ.get("CTC_ACCURACY_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "ctc_accuracy.json")
    try:
        rows = json.load(open(path))
    except (OSError, ValueError):
        rows = {}
    rows[route] = row
    json.dump(rows, open(path, "w"), indent=1, sort_keys=True)


class CtcCall:
    """The tensors of one call; the workspace and the gradient buffer start as 0xFF bytes.  `offset_floats` shifts acts and grads off
    their 16-byte alignment."""

    def __init__(self, acts, labels, il, ll, blank=0, offset_floats=0, stream=None):
        pkg.build()
        self.lib = _lib.load_ctc()
        B, T, V = acts.shape
        self.shape = (B, T, V)
        self.U = labels.shape[1] + 1
        d = torch.device(DEV)
        abuf = torch.zeros(acts.size + 8, dtype=torch.float32, device=d)
        self.acts = abuf[offset_floats: offset_floats + acts.size]
        self.acts.copy_(torch.as_tensor(acts.reshape(-1), device=d))
        self.labels = torch.as_tensor(np.ascontiguousarray(labels, np.int32), device=d)
        self.il = torch.as_tensor(np.asarray(il, np.int32), device=d)
        self.ll = torch.as_tensor(np.asarray(ll, np.int32), device=d)
        self.ws = torch.full((_lib.ctc_workspace_bytes(T, self.U, B),), 0xFF, dtype=torch.uint8, device=d)
        self.costs = torch.full((B,), float("nan"), device=d)
        self.gbytes = torch.full(((acts.size + 8) * 4,), 0xFF, dtype=torch.uint8, device=d)
        self.grads = self.gbytes.view(torch.float32)[offset_floats: offset_floats + acts.size]
        self.opts = _lib.make_options((stream or torch.cuda.current_stream()).cuda_stream, blank, T, self.U)

    def enqueue(self, scale=None, costs=True, grads=True):
        B, T, V = self.shape
        return self.lib.compute_rnnt_ctc_loss(
            self.acts.data_ptr(), self.grads.data_ptr() if grads else None, self.labels.data_ptr(), self.ll.data_ptr(),
            self.il.data_ptr(), scale.data_ptr() if scale is not None else None, V, B, self.costs.data_ptr() if costs else None,
            self.ws.data_ptr(), self.opts)

    def run(self, scale=None, costs=True, grads=True):
        """Poisons what the call is to write (the workspace too when the call runs the forward), runs it, returns (costs, grads)."""
        if grads:
            self.gbytes.fill_(0xFF)
        if costs:
            self.ws.fill_(0xFF)
            self.costs.fill_(float("nan"))
        scale_t = None if scale is None else torch.tensor(np.asarray(scale), dtype=torch.float32, device=DEV)
        assert self.enqueue(scale_t, costs, grads) == 0
        return self.result()

    def result(self):
        torch.cuda.synchronize()
        return self.costs.cpu().numpy().astype(np.float64), self.grads.cpu().numpy().reshape(self.shape)


def _check(route, c, g, ref, il, scale=None):
    """costs / gradients against the reference `ref` with the fixed bars; exact zeros on padded frames and for utterances
    without a path; returns the maxima."""
    c_ref, g_ref = ref
    B = len(c_ref)
    cs = np.ones(B) if scale is None else np.abs(np.broadcast_to(np.asarray(scale, np.float64), (B,)))
    fin = np.isfinite(c_ref)
    assert np.array_equal(c[~fin], c_ref[~fin])  # an utterance without a path: +inf exactly
    dc = np.abs(c[fin] - c_ref[fin]) / np.maximum(1.0, np.abs(c_ref[fin]))
    assert np.isfinite(g).all()
    dg = np.array([np.abs(g[b] - g_ref[b]).max() / max(cs[b], 1e-30) for b in range(B)])
    zeros_ok = all(not g[b, int(il[b]):].any() for b in range(B)) and all(not g[b].any() for b in range(B) if not fin[b])
    _record(route, cost_rel=dc.max() if dc.size else 0.0, grad_abs_over_scale=dg.max())
    assert dc.size == 0 or dc.max() <= CTOL
    assert dg.max() <= GTOL
    assert zeros_ok
    return dc, dg


def _batch(utts, V, seed, sigma=1.0):
    """A ragged batch from [(T, labels)]: (acts, labels, il, ll)."""
    rng = np.random.default_rng(seed)
    T, Lmax = max(t for t, _ in utts), max(1, max(len(y) for _, y in utts))
    acts = (sigma * rng.normal(size=(len(utts), T, V))).astype(np.float32)
    labels = np.ones((len(utts), Lmax), np.int32)
    for b, (_, y) in enumerate(utts):
        labels[b, : len(y)] = y
    return acts, labels, np.array([t for t, _ in utts], np.int32), np.array([len(y) for _, y in utts], np.int32)


# ---- lattice edges ------------------------------------------------------------------------------------------------------
EDGES = [
    ("T1_L0", 1, []), ("T1_L1", 1, [2]), ("T7_L0", 7, []),
    ("T_eq_L_single_path", 6, [1, 2, 3, 4, 1, 2]),
    ("T_eq_L_one_repeat_infeasible", 6, [1, 2, 2, 4, 1, 2]),
    ("T_eq_L_plus_repeats", 8, [1, 2, 2, 4, 4, 2]),
    ("all_equal", 21, [3] * 9),
    ("abab", 40, [1, 2] * 17),
    ("first_middle_last", 14, [4, 1, 2, 4, 3, 1, 4]),
]


def test_lattice_edges_in_one_ragged_batch_and_alone():
    utts = [(T, y) for _, T, y in EDGES]
    acts, labels, il, ll = _batch(utts, 5, seed=1)
    ref = cc.loss_and_grad(acts, labels, il, ll)
    assert np.isinf(ref[0][4]) and np.isfinite(np.delete(ref[0], 4)).all()
    c, g = CtcCall(acts, labels, il, ll).run()
    _check("edges_batch_V5", c, g, ref, il)
    for b, (name, T, y) in enumerate(EDGES):  # each on the geometry of its own shape, bit for bit what the batch gave it
        c1, g1 = CtcCall(acts[b: b + 1, :T], labels[b: b + 1, : max(len(y), 1)], il[b: b + 1], ll[b: b + 1]).run()
        _check("edge_" + name, c1, g1, (ref[0][b: b + 1], ref[1][b: b + 1, :T]), il[b: b + 1])
        assert np.array_equal(c1, c[b: b + 1]), name
        assert np.array_equal(g1[0], g[b, :T]), name


# ---- hand-over boundaries of the sweeps ---------------------------------------------------------------------------------
_WAVE, _SWITCH, _WIDE = cc.tier_boundaries()
WAVE_POSITIONS = sorted({p + d for p in [CONST["kCtcWaveThreads"]] + _WAVE + [_SWITCH] for d in (-1, 0, 1)})
WIDE_POSITIONS = sorted({p + d for p in _WIDE for d in (-1, 0, 1)})


def _tier_case(P, seed):
    """One utterance with L + 1 = P positions, T = the fewest frames with a path + 3, V = 5."""
    L = P - 1
    rng = np.random.default_rng(seed)
    y = cc.random_labels(rng, L, 5, repeat_prob=0.05)
    T = cc.min_frames(y) + 3
    acts = rng.normal(size=(1, T, 5)).astype(np.float32)
    return acts, y[None, :], np.array([T], np.int32), np.array([L], np.int32)


@pytest.mark.parametrize("P", WAVE_POSITIONS)
def test_one_wavefront_tiers(P):
    """L + 1 = 63, 64, 65 and +-1 around every positions-per-thread tier of the one-wavefront sweep and its switch to a workgroup."""
    acts, labels, il, ll = _tier_case(P, seed=P)
    c, g = CtcCall(acts, labels, il, ll).run()
    _check(f"tier_P{P}", c, g, cc.loss_and_grad(acts, labels, il, ll), il)


@pytest.mark.parametrize("P", WIDE_POSITIONS)
def test_workgroup_tiers(P):
    """+-1 around every positions-per-thread tier of the workgroup sweep (the reference: torch's float64 CPU CTC)."""
    acts, labels, il, ll = _tier_case(P, seed=P)
    c, g = CtcCall(acts, labels, il, ll).run()
    _check(f"tier_P{P}", c, g, cc.torch_ctc(acts, labels, il, ll), il)


def test_the_longest_label_sequence():
    """L = 8191 (maxU = 8192), T = L + 4, V = 3, no repeats: a workspace of about 2 GB; the reference is torch's float64 CPU CTC."""
    L, V = 8191, 3
    T = L + 4
    y = np.tile(np.array([1, 2], np.int32), L // 2 + 1)[:L]
    acts = np.random.default_rng(8191).normal(size=(1, T, V)).astype(np.float32)
    il, ll = np.array([T], np.int32), np.array([L], np.int32)
    c, g = CtcCall(acts, y[None, :], il, ll).run()
    _check("longest_L8191_T8195_V3", c, g, cc.torch_ctc(acts, y[None, :], il, ll), il)


# ---- row and gradient tiles ---------------------------------------------------------------------------------------------
ROW_PASS = 64 * CONST["kCtcRowVec"]  # elements per pass of the row kernel on aligned rows; 64 on the scalar route
VOCABS = sorted({2, 3, 5, 28, 31, 32, 33, 63, 64, 65, ROW_PASS - 1, ROW_PASS, ROW_PASS + 1, CONST["kCtcGradTile"] + 1,
                 CONST["kCtcGradTile"] + 4})


@pytest.mark.parametrize("V", VOCABS)
def test_vocabulary_routes(V):
    for blank in sorted({0, V - 1, V // 2}):
        acts, labels, il, ll = cc.case(2, 12, 5, V, seed=V, blank=blank)
        il[1], ll[1] = 9, 3
        assert not (labels == blank).any()
        c, g = CtcCall(acts, labels, il, ll, blank=blank).run()
        _check(f"vocab_V{V}_blank{blank}", c, g, cc.loss_and_grad(acts, labels, il, ll, blank=blank), il)


@pytest.mark.parametrize("V", [5, 31, 32, ROW_PASS + 1])
def test_unaligned_rows(V):
    """acts and grads one float off their 16-byte alignment: the scalar routes of the row, gradient and greedy kernels."""
    acts, labels, il, ll = cc.case(2, 12, 5, V, seed=300 + V)
    il[0] = 10
    c, g = CtcCall(acts, labels, il, ll, offset_floats=1).run()
    _check(f"unaligned_V{V}", c, g, cc.loss_and_grad(acts, labels, il, ll), il)
    c2, g2 = CtcCall(acts, labels, il, ll, offset_floats=0).run()
    if V % 4:  # the same route on both: the same bits
        assert np.array_equal(c, c2) and np.array_equal(g, g2)


# ---- ranges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [1.0, 4.0, 8.0])
def test_logit_ranges(sigma):
    acts, labels, il, ll = cc.case(3, 120, 30, 28, seed=int(sigma), sigma=sigma)
    il[1], ll[1] = 97, 22
    c, g = CtcCall(acts, labels, il, ll).run()
    _check(f"range_B3_T120_L30_V28_sigma{sigma:g}", c, g, cc.loss_and_grad(acts, labels, il, ll), il)


def test_trained_like_posteriors():
    acts, labels, il, ll = cc.trained_like_case(4, 600, 150, 28, seed=21)
    c, g = CtcCall(acts, labels, il, ll).run()
    _check("trained_B4_T600_L150_V28", c, g, cc.loss_and_grad(acts, labels, il, ll), il)


def test_a_long_wide_utterance():
    acts, labels, il, ll = cc.case(1, 1500, 300, 1024, seed=1500, sigma=8.0)
    c, g = CtcCall(acts, labels, il, ll).run()
    _check("long_B1_T1500_L300_V1024_sigma8", c, g, cc.loss_and_grad(acts, labels, il, ll), il)


# ---- protocol -----------------------------------------------------------------------------------------------------------
def _ragged():
    acts, labels, il, ll = cc.case(5, 40, 12, 28, seed=77)
    il[:], ll[:] = [40, 31, 9, 40, 17], [12, 7, 12, 0, 5]
    labels[2, :12] = [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]  # 18 frames needed, 9 given: no path
    return acts, labels, il, ll


def test_ragged_batch_and_each_utterance_alone():
    acts, labels, il, ll = _ragged()
    scale = np.array([0.5, -1.0, 2.0, 1.0, 0.25])
    k = CtcCall(acts, labels, il, ll)
    c, g = k.run(scale=scale)
    assert c[2] == np.inf and not g[2].any()
    _check("ragged_B5_T40_L12_V28", c, g, cc.loss_and_grad(acts, labels, il, ll, scale), il, scale)
    c2, g2 = k.run(scale=scale)  # two runs: the same bits
    assert np.array_equal(c, c2) and np.array_equal(g, g2)
    for b in range(5):  # the same utterance alone, in the same tensor shape: the same bits
        c1, g1 = CtcCall(acts[b: b + 1], labels[b: b + 1], il[b: b + 1], ll[b: b + 1]).run(scale=scale[b: b + 1])
        assert np.array_equal(c1[0], c[b]) and np.array_equal(g1[0], g[b]), b


def test_split_calls_are_the_combined_call():
    acts, labels, il, ll = _ragged()
    s1, s2 = np.array([0.5, -1.0, 2.0, 1.0, 0.25]), np.array([3.0, 1.0, -0.5, 0.125, 1.0])
    k = CtcCall(acts, labels, il, ll)
    c, g1 = k.run(scale=s1)
    _, g2 = k.run(scale=s2)
    _, g0 = k.run()
    cf, _ = k.run(grads=False)  # forward alone (poisoned workspace)
    assert np.array_equal(cf, c)
    for scale, want in ((s1, g1), (s2, g2), (None, g0), (s1, g1)):  # gradient passes alone, from the workspace that forward left
        _, gb = k.run(scale=scale, costs=False)
        assert np.array_equal(gb, want)
    assert np.array_equal(k.result()[0], c)  # the gradient pass does not touch the costs
    _check("cost_scale_null", c, g0, cc.loss_and_grad(acts, labels, il, ll), il)


def test_a_non_default_stream():
    acts, labels, il, ll = _ragged()
    c, g = CtcCall(acts, labels, il, ll).run()
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        k = CtcCall(acts, labels, il, ll, stream=side)
        side.wait_stream(torch.cuda.default_stream())
        assert k.enqueue() == 0
    side.synchronize()
    cs, gs = k.result()
    assert np.array_equal(cs, c) and np.array_equal(gs, g)


@pytest.mark.parametrize("what,value", [("T", 0), ("T", 41), ("L", -1), ("L", 13), ("blank_label", 0)])
def test_invalid_utterances_are_nan_and_leave_their_neighbours_alone(what, value):
    """maxT = 40, maxU = 13: T_b in {0, maxT + 1}, L_b in {-1, maxU}, or a label equal to the blank."""
    acts, labels, il, ll = _ragged()
    c0, g0 = CtcCall(acts, labels, il, ll).run()
    il_bad, ll_bad, labels_bad = il.copy(), ll.copy(), labels.copy()
    if what == "T":
        il_bad[1] = value
    elif what == "L":
        ll_bad[1] = value
    else:
        labels_bad[1, 3] = value
    c, g = CtcCall(acts, labels_bad, il_bad, ll_bad).run()
    assert np.isnan(c[1])
    Tc = min(max(int(il_bad[1]), 1), 40)  # clamped into the tensor
    assert np.isnan(g[1, :Tc]).all() and not g[1, Tc:].any()
    keep = [0, 2, 3, 4]
    assert np.array_equal(c[keep], c0[keep]) and np.array_equal(g[keep], g0[keep])
    c2, _ = CtcCall(acts, labels, il, ll).run()  # the process goes on
    assert np.array_equal(c2, c0)


# ---- greedy -------------------------------------------------------------------------------------------------------------
def _greedy_gpu(acts, il, blank=0, frames=True, offset_floats=0):
    pkg.build()
    lib = _lib.load_ctc()
    B, T, V = acts.shape
    d = torch.device(DEV)
    abuf = torch.zeros(acts.size + 8, dtype=torch.float32, device=d)
    a = abuf[offset_floats: offset_floats + acts.size]
    a.copy_(torch.as_tensor(acts.reshape(-1), device=d))
    il_t = torch.as_tensor(np.asarray(il, np.int32), device=d)
    tokens = torch.full((B, T), -7, dtype=torch.int32, device=d)
    tframes = torch.full((B, T), -7, dtype=torch.int32, device=d)
    lengths = torch.full((B,), -7, dtype=torch.int32, device=d)
    opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, blank, T, 0)  # (maxU is not read)
    assert lib.compute_rnnt_ctc_greedy(a.data_ptr(), il_t.data_ptr(), V, B, tokens.data_ptr(), tframes.data_ptr() if frames else None,
                                       lengths.data_ptr(), opts) == 0
    torch.cuda.synchronize()
    return tokens.cpu().numpy(), tframes.cpu().numpy(), lengths.cpu().numpy()


def _greedy_check(acts, il, blank=0, **kw):
    want = cc.greedy(acts, il, blank)
    got = _greedy_gpu(acts, il, blank, **kw)
    for w, g_ in zip(want, got):
        assert np.array_equal(w, g_)
    for b in range(acts.shape[0]):
        assert (got[0][b, got[2][b]:] == -1).all() and (got[1][b, got[2][b]:] == -1).all()
    return got


@pytest.mark.parametrize("name,script,blank,V", cc.GREEDY_SCRIPTS, ids=[s[0] for s in cc.GREEDY_SCRIPTS])
def test_greedy_scripts_are_the_mirror_bit_for_bit(name, script, blank, V):
    acts, il = cc.scripted_logits(script, V)
    tokens, _, lengths = _greedy_check(acts, il, blank)
    mirror = pkg.ctc_greedy_decode(torch.tensor(acts), torch.tensor(il), blank, return_frames=True)
    device = pkg.ctc_greedy_decode(torch.tensor(acts, device=DEV), torch.tensor(il, device=DEV), blank, return_frames=True)
    for m, d in zip(mirror, device):
        assert d.dtype == torch.int32 and np.array_equal(m.numpy(), d.cpu().numpy())
    t_only, _, l_only = _greedy_gpu(acts, il, blank, frames=False)  # token_frames == NULL
    assert np.array_equal(t_only, tokens) and np.array_equal(l_only, lengths)


@pytest.mark.parametrize("V", [2, 5, 4096])
def test_greedy_vocabularies_chunks_and_a_ragged_batch(V):
    """T across the compaction chunk and twice the chunk, +-1, as the lengths of one ragged batch (and 0 and 1)."""
    C = CONST["kCtcGreedyChunk"]
    il = np.array([C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 0, 1], np.int32)
    rng = np.random.default_rng(V)
    acts = rng.normal(size=(len(il), 2 * C + 1, V)).astype(np.float32)
    acts[:, :, 0] += 0.5  # (some blanks)
    acts[0, :, :] = acts[0, :1, :]  # one symbol on every frame: one token, or none
    acts[1, :, 1] += 20.0 * (np.arange(2 * C + 1) % 2)  # symbol 1 on every other frame: the most tokens a sequence can hold
    for blank in (0, V - 1):
        _, _, lengths = _greedy_check(acts, il, blank)
        assert lengths[6] == 0 and lengths[0] <= 1
        if V % 4:
            _greedy_check(acts, il, blank, offset_floats=1)


# ---- the Python surface -------------------------------------------------------------------------------------------------
def test_autograd_on_the_device_is_the_cpu_mirror():
    acts, labels, il, ll = _ragged()
    w = np.array([0.5, -1.5, 2.0, 1.0, 0.25])
    out = []
    for dev in ("cpu", DEV):
        x = torch.tensor(acts, device=dev, requires_grad=True)
        costs = pkg.ctc_loss(x, torch.tensor(labels, device=dev), torch.tensor(il, device=dev), torch.tensor(ll, device=dev),
                             zero_infinity=True)
        (torch.tensor(w, dtype=torch.float32, device=dev) * costs).sum().backward()
        out.append((costs.detach().cpu().numpy().astype(np.float64), x.grad.cpu().numpy().astype(np.float64)))
    (c_cpu, g_cpu), (c_dev, g_dev) = out
    assert c_dev[2] == 0 and c_cpu[2] == 0  # zero_infinity
    ref = cc.loss_and_grad(acts, labels, il, ll, w)
    ref[0][2] = 0.0
    _check("autograd_device", c_dev, g_dev, ref, il, w)
    assert np.abs(c_dev - c_cpu).max() <= CTOL * np.abs(c_cpu).max() and np.abs(g_dev - g_cpu).max() <= GTOL * np.abs(w).max()
    c1, g1 = pkg.ctc_loss_and_grad(torch.tensor(acts, device=DEV), torch.tensor(labels, device=DEV), torch.tensor(il, device=DEV),
                                   torch.tensor(ll, device=DEV))
    torch.cuda.synchronize()
    _check("loss_and_grad", c1.cpu().numpy().astype(np.float64), g1.cpu().numpy(), cc.loss_and_grad(acts, labels, il, ll), il)
    loss = pkg.CTCLoss(reduction="mean", zero_infinity=True)(torch.tensor(acts, device=DEV), torch.tensor(labels, device=DEV),
                                                              torch.tensor(il, device=DEV), torch.tensor(ll, device=DEV))
    assert abs(float(loss) - ref[0].mean()) <= CTOL * max(1.0, np.abs(ref[0]).max())


def test_a_hybrid_train_step_on_the_device():
    from tests.test_model import small_hp

    torch.manual_seed(0)
    dev = torch.device(DEV)
    hp = small_hp()
    m = pkg.Transducer(hp, ctc_weight=0.3).to(dev)
    batch = pkg.synthetic_batch(hp, batch=6, frames=40, max_labels=7, device=dev, seed=3)
    m.train()
    costs = m.loss(*batch)
    assert costs.shape == (6,) and torch.isfinite(costs).all()
    costs.mean().backward()
    gw, gb = m.ctc_head.weight.grad, m.ctc_head.bias.grad
    assert torch.isfinite(gw).all() and torch.isfinite(gb).all() and float(gw.abs().max()) > 0 and float(gb.abs().max()) > 0
    m.eval()
    with torch.no_grad():
        plain = pkg.Transducer(hp).to(dev)
        plain.load_state_dict(m.state_dict(), strict=False)
        plain.eval()
        assert torch.equal(m.loss(*batch), plain.loss(*batch))  # eval: the transducer's NLL alone
    before = m.ctc_head.weight.detach().clone()
    out = pkg.TrainStep(m, global_batch=6)(*batch)
    assert np.isfinite(out["loss"]) and not torch.equal(before, m.ctc_head.weight.detach())
    tokens, lengths = m.ctc_decode(batch[0], batch[2])
    assert tokens.shape[0] == 6 and tokens.dtype == torch.int32 and int(lengths.min()) >= 0
