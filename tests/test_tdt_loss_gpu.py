"""GPU tests of the token-and-duration (TDT) transducer loss (include/rnnt_tdt.h compute_rnnt_loss_tdt) against the float64
restatement of tests/tdt_cases.py.

Bars: the op's own fixed ones (include/rnnt.h) -- costs within 1e-4 max(1, |cost|), gradients within 1e-4 |cost_scale| absolute.
Padded cells, cells no path crosses and utterances without a path are exact zeros.  Every call through the C ABI gets a gradient
buffer and a workspace filled with 0xFF bytes (a gradient-only call: the workspace its forward left).
The measured maxima are printed and, with TDT_ACCURACY_DIR set, collected in tdt_accuracy.json in that directory (the maxima per group are
kept in profiles/tdt_loss_notes.md)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib
from tests import tdt_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTOL = GTOL = 1e-4
D5 = [0, 1, 2, 3, 4]
D8 = [0, 1, 2, 3, 4, 5, 6, 8]  # D = 8, dmax = 8, a gap
DURATION_SETS = [D5, [1, 2], [0, 1], [1], [0, 2], D8]


def _record(route, **figures):
    row = {k: float(v) for k, v in figures.items()}
    print(route, row)
    out = os.environ.get("TDT_ACCURACY_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "tdt_accuracy.json")
    try:
        rows = json.load(open(path))
    except (OSError, ValueError):
        rows = {}
    rows[route] = row
    json.dump(rows, open(path, "w"), indent=1, sort_keys=True)


class TdtCall:
    """The tensors of one call; the workspace and the gradient buffer start as 0xFF bytes."""

    def __init__(self, acts, labels, il, ll, durations, blank=0, sigma=0.0, grad_offset_floats=0, stream=None):
        pkg.build()
        self.lib = _lib.load_tdt()
        B, T, U, R = acts.shape
        self.shape = (B, T, U, R)
        self.D = len(durations)
        self.dur = (ctypes.c_int * self.D)(*durations)
        self.sigma = sigma
        d = torch.device(DEV)
        self.acts = torch.as_tensor(acts, device=d).contiguous()
        self.labels = torch.as_tensor(labels, device=d).contiguous()
        self.il = torch.as_tensor(il, device=d)
        self.ll = torch.as_tensor(ll, device=d)
        self.ws = torch.full((_lib.tdt_workspace_bytes(T, U, B, self.D),), 0xFF, dtype=torch.uint8, device=d)
        self.costs = torch.full((B,), float("nan"), device=d)
        self.gbytes = torch.full(((acts.size + 8) * 4,), 0xFF, dtype=torch.uint8, device=d)
        self.grads = self.gbytes.view(torch.float32)[grad_offset_floats: grad_offset_floats + acts.size]
        self.opts = _lib.make_options((stream or torch.cuda.current_stream()).cuda_stream, blank, T, U)

    def enqueue(self, scale=None, costs=True, grads=True):
        B, T, U, R = self.shape
        return self.lib.compute_rnnt_loss_tdt(
            self.acts.data_ptr(), self.grads.data_ptr() if grads else None, self.labels.data_ptr(), self.ll.data_ptr(),
            self.il.data_ptr(), scale.data_ptr() if scale is not None else None, R - self.D, self.dur, self.D, self.sigma, B,
            self.costs.data_ptr() if costs else None, self.ws.data_ptr(), self.opts)

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


def _check(route, c, g, ref, scale=None, crossed=None):
    """costs / gradients against the restatement `ref` with the fixed bars; every element written (no poison, no NaN); exact zeros
    wherever the restatement has a whole cell of zeros (padding, no path, cells no path crosses)."""
    c_ref, g_ref = ref
    B = len(c_ref)
    cs = np.ones(B) if scale is None else np.abs(np.broadcast_to(np.asarray(scale, np.float64), (B,)))
    fin = np.isfinite(c_ref)
    assert np.array_equal(c[~fin], c_ref[~fin])  # an utterance without a path: +inf exactly
    dc = np.abs(c[fin] - c_ref[fin]) / np.maximum(1.0, np.abs(c_ref[fin]))
    assert np.isfinite(g).all()  # the 0xFF poison is a NaN
    dg = np.array([np.abs(g[b] - g_ref[b]).max() / max(cs[b], 1e-30) for b in range(B)])
    off = ~g_ref.any(axis=-1) if crossed is None else ~crossed
    zeros_ok = not g[off].any()
    _record(route, cost_rel=dc.max() if dc.size else 0.0, grad_abs_over_scale=dg.max())
    assert dc.size == 0 or dc.max() <= CTOL
    assert dg.max() <= GTOL
    assert zeros_ok
    return dc, dg


# ---- lane and wave edges ------------------------------------------------------------------------------------------------
EDGE_L = [62, 63, 64, 65, 127, 128, 129, 255, 256, 257]


def test_lane_and_wave_edges():
    """One utterance per width in ONE batch (maxU = 258: five waves of columns), T_b = 6: each utterance's last column on, next to
    and across a multiple of 64, where the label edges cross from one wave's lanes to the next."""
    lengths = [(6, L) for L in EDGE_L]
    acts, labels, il, ll = tc.ragged_case(lengths, 5, 5, seed=10)
    c, g = TdtCall(acts, labels, il, ll, D5).run()
    assert np.isfinite(c).all()
    _check("edges_B10_T6_V5_d5", c, g, tc.loss_and_grad(acts, labels, il, ll, D5))


def test_widest_lattice():
    """maxU = 1024, the op's limit: L_b = 1022 and 1023, T_b = 4; sixteen waves and the whole 80 KB ring."""
    acts, labels, il, ll = tc.ragged_case([(4, 1022), (4, 1023)], 5, 5, seed=11)
    c, g = TdtCall(acts, labels, il, ll, D5).run()
    assert np.isfinite(c).all()
    _check("widest_B2_T4_U1024_V5_d5", c, g, tc.loss_and_grad(acts, labels, il, ll, D5))


# ---- frame edges against dmax -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("durations", DURATION_SETS, ids=[str(d) for d in DURATION_SETS])
def test_frame_edges(durations):
    """T_b in {1, 2, dmax, dmax+1, dmax+2, 2 dmax+3} x L_b in {0, 1, 5} in ONE batch: the terminal rule t + d == T, the wrap of the
    ring, and utterances without a path beside feasible ones."""
    dmax = durations[-1]
    lengths = [(T, L) for T in sorted({1, 2, dmax, dmax + 1, dmax + 2, 2 * dmax + 3}) for L in (0, 1, 5)]
    acts, labels, il, ll = tc.ragged_case(lengths, 6, len(durations), seed=20 + dmax)
    ref = tc.loss_and_grad(acts, labels, il, ll, durations)
    feasible = np.isfinite(ref[0])
    if durations in ([1, 2], [1], [0, 2]):
        assert not feasible.all()
    assert feasible.any()
    c, g = TdtCall(acts, labels, il, ll, durations).run()
    _check(f"frames_d{'_'.join(map(str, durations))}", c, g, ref, crossed=tc.crossed_mask(acts, labels, il, ll, durations))
    assert not g[~feasible].any()


# ---- row layout ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,D", [(4, 2), (4, 3), (3, 5), (4, 5), (5, 8), (1030, 5)])
def test_row_layout(V, D):
    """V + D in {6, 7, 8, 9, 13}: 16-byte-aligned rows (8) and unaligned ones, a duration block that straddles a 16-byte piece; and
    V = 1030: several pieces per lane.  The blank at 0, at V - 1 and in the middle; sigma 0 and 0.05."""
    durations = {2: [1, 2], 3: [0, 1, 2], 5: D5, 8: D8}[D]
    for blank, sigma in ((0, 0.0), (V - 1, 0.05), (V // 2, 0.05)):
        acts, labels, il, ll = tc.ragged_case([(12, 5), (9, 3)], V, D, seed=V + D, blank=blank)
        assert not (labels == blank).any()
        c, g = TdtCall(acts, labels, il, ll, durations, blank=blank, sigma=sigma).run()
        _check(f"row_V{V}_D{D}_blank{blank}_sigma{sigma}", c, g, tc.loss_and_grad(acts, labels, il, ll, durations, blank, sigma))


@pytest.mark.parametrize("V,D", [(3, 5), (4, 5)])
def test_unaligned_gradient_buffer(V, D):
    """A gradient buffer that is 4-byte aligned only, with rows of 8 floats (the 16-byte route must step aside) and of 9."""
    acts, labels, il, ll = tc.ragged_case([(12, 5), (9, 3)], V, D, seed=7)
    c, g = TdtCall(acts, labels, il, ll, D5, grad_offset_floats=1).run()
    _check(f"unaligned_grads_V{V}_D{D}", c, g, tc.loss_and_grad(acts, labels, il, ll, D5))


# ---- numerics -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_case(kind):
    if kind == "n08":
        case = tc.full_case(2, 600, 20, 8, 5, seed=30, scale=8.0)
    else:
        case = tc.trained_like_case(2, 100, 30, 8, D5, seed=31)
    return case, {s: tc.loss_and_grad(*case, D5, sigma=s) for s in (0.0, 0.05)}


@pytest.mark.parametrize("sigma", [0.0, 0.05])
@pytest.mark.parametrize("kind", ["n08", "trained"])
def test_long_paths(kind, sigma):
    """8 x N(0,1) logits at T = 600 (|alpha|, |beta| in the thousands: why they are stored as float64) and trained-like peaked
    posteriors at T = 100, L = 30."""
    (acts, labels, il, ll), refs = _long_case(kind)
    c, g = TdtCall(acts, labels, il, ll, D5, sigma=sigma).run()
    assert np.isfinite(c).all()
    _check(f"long_{kind}_sigma{sigma}", c, g, refs[sigma])


# ---- call modes ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ragged5():
    case = tc.ragged_case([(20, 8), (20, 0), (1, 0), (1, 2), (7, 8)], 7, 5, seed=40)
    return case, tc.loss_and_grad(*case, D5, sigma=0.05)


def test_call_modes():
    (acts, labels, il, ll), ref = _ragged5()
    s1, s2 = np.array([0.5, -1.0, 2.0, 1.0, 0.25]), np.array([-2.0, 0.2, 1.0, 3.0, 1.0])
    k = TdtCall(acts, labels, il, ll, D5, sigma=0.05)
    c, g = k.run()  # both in one call, cost_scale = NULL
    _check("modes_both_null_scale", c, g, ref)
    cf, _ = k.run(grads=False)  # forward only (poisoned workspace): the ONE forward of the gradient-only calls below
    assert np.array_equal(cf, c)
    only = {}
    for name, s in (("s1", s1), ("s2", s2), ("s1_again", s1)):  # gradient only, back to back, nothing in between
        _, only[name] = k.run(scale=s, costs=False)
        _check(f"modes_grad_only_{name}", c, only[name], (ref[0], ref[1] * s[:, None, None, None]), s)
    assert np.array_equal(only["s1_again"], only["s1"])  # a gradient pass leaves the workspace as it found it
    assert np.array_equal(k.result()[0], c)  # and does not touch the costs
    for name, s in (("s1", s1), ("s2", s2)):  # the combined call with the same scale: the same bits
        cc, gc = k.run(scale=s)
        assert np.array_equal(cc, c) and np.array_equal(gc, only[name])


def test_side_stream():
    (acts, labels, il, ll), ref = _ragged5()
    c, g = TdtCall(acts, labels, il, ll, D5, sigma=0.05).run()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        k = TdtCall(acts, labels, il, ll, D5, sigma=0.05, stream=side)
        assert k.enqueue() == 0
    side.synchronize()
    cs, gs = k.result()
    assert np.array_equal(cs, c) and np.array_equal(gs, g)


# ---- padding ------------------------------------------------------------------------------------------------------------
def test_ragged_batch_padding_and_poison():
    (acts, labels, il, ll), ref = _ragged5()
    c, g = TdtCall(acts, labels, il, ll, D5, sigma=0.05).run()
    _check("ragged_B5_T20_U9_V7_d5", c, g, ref)
    for b in range(5):
        assert not g[b, il[b]:].any() and not g[b, :, ll[b] + 1:].any()
    assert np.isfinite(c[3])  # (T, L) = (1, 2): two labels stacked on the one frame


@pytest.mark.parametrize("what,value", [("T", 0), ("T", 13), ("L", -1), ("L", 6)])
def test_out_of_range_lengths(what, value):
    """maxT = 12, maxU = 6: T_b in {0, maxT + 1}, L_b in {-1, maxU}.  That utterance is NaN, its neighbours are not touched."""
    acts, labels, il, ll = tc.ragged_case([(9, 3), (12, 5), (12, 5)], 6, 5, seed=60)
    il_bad, ll_bad = il.copy(), ll.copy()
    (il_bad if what == "T" else ll_bad)[1] = value
    c, g = TdtCall(acts, labels, il_bad, ll_bad, D5).run()
    assert np.isnan(c[1])
    Tc, Lc = min(max(int(il_bad[1]), 1), 12), min(max(int(ll_bad[1]), 0), 5)  # clamped into the tensor
    assert np.isnan(g[1, :Tc, : Lc + 1]).all()
    assert not g[1, Tc:].any() and not g[1, :, Lc + 1:].any()
    ref = tc.loss_and_grad(acts, labels, il, ll, D5)
    keep = [0, 2]
    _check(f"bad_{what}{value}", c[keep], g[keep], (ref[0][keep], ref[1][keep]))


def test_out_of_range_labels_are_clamped():
    acts, labels, il, ll = tc.ragged_case([(9, 3), (12, 5)], 6, 5, seed=61)
    wild = labels.copy()
    wild[1, 0], wild[1, 2] = -7, 1000
    c, g = TdtCall(acts, wild, il, ll, D5).run()
    _check("clamped_labels", c, g, tc.loss_and_grad(acts, np.clip(wild, 0, 5), il, ll, D5))


# ---- determinism --------------------------------------------------------------------------------------------------------
def test_same_bits_twice_and_alone():
    (acts, labels, il, ll), _ = _ragged5()
    k = TdtCall(acts, labels, il, ll, D5, sigma=0.05)
    c, g = k.run()
    c2, g2 = k.run()
    assert np.array_equal(c, c2) and np.array_equal(g, g2)
    for b in (0, 3, 4):  # an utterance alone, in a tensor of the batch's shape, and inside the batch
        ca, ga = TdtCall(acts[b: b + 1], labels[b: b + 1], il[b: b + 1], ll[b: b + 1], D5, sigma=0.05).run()
        assert np.array_equal(ca[0], c[b]) and np.array_equal(ga[0], g[b])


# ---- the Python surface -------------------------------------------------------------------------------------------------
def test_python_surface():
    pkg.build()
    (acts, labels, il, ll), ref = _ragged5()
    t = lambda a: torch.tensor(a, device=DEV)  # noqa: E731
    x = torch.tensor(acts, device=DEV, requires_grad=True)
    costs = pkg.rnnt_loss_tdt(x, t(labels), t(il), t(ll), D5, sigma=0.05)
    costs.sum().backward()
    c1, g1 = pkg.rnnt_loss_tdt_and_grad(t(acts), t(labels), t(il), t(ll), D5, sigma=0.05)
    torch.cuda.synchronize()
    assert costs.dtype == torch.float32
    assert np.array_equal(costs.detach().cpu().numpy(), c1.cpu().numpy()) and np.array_equal(x.grad.cpu().numpy(), g1.cpu().numpy())
    _check("python_and_grad", c1.cpu().numpy().astype(np.float64), g1.cpu().numpy(), ref)
    # the CPU mirror is the same function
    cm, gm = pkg.rnnt_loss_tdt_and_grad(torch.tensor(acts), torch.tensor(labels), torch.tensor(il), torch.tensor(ll), D5, sigma=0.05)
    _check("python_vs_mirror", c1.cpu().numpy().astype(np.float64), g1.cpu().numpy(), (cm.numpy(), gm.numpy()))
    # a weighted sum through autograd, and the module's reductions
    w = np.array([0.5, -1.5, 2.0, 1.0, 0.25])
    x = torch.tensor(acts, device=DEV, requires_grad=True)
    (torch.tensor(w, dtype=torch.float32, device=DEV) * pkg.rnnt_loss_tdt(x, t(labels), t(il), t(ll), D5, sigma=0.05)).sum().backward()
    torch.cuda.synchronize()
    _check("autograd_weighted", ref[0], x.grad.cpu().numpy(), (ref[0], ref[1] * w[:, None, None, None]), w)
    x = torch.tensor(acts, device=DEV, requires_grad=True)
    loss = pkg.TDTLoss(D5, sigma=0.05, reduction="mean")(x, t(labels), t(il), t(ll))
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - ref[0].mean()) <= CTOL * max(1.0, abs(ref[0].mean()))
    _check("module_mean", ref[0], x.grad.cpu().numpy(), (ref[0], ref[1] / 5), 1.0 / 5)
    total = pkg.TDTLoss(D5, sigma=0.05, reduction="sum")(t(acts), t(labels), t(il), t(ll))
    assert abs(float(total) - ref[0].sum()) <= CTOL * max(1.0, abs(ref[0].sum()))
    assert pkg.TDTLoss(D5, sigma=0.05)(t(acts), t(labels), t(il), t(ll)).shape == (5,)
