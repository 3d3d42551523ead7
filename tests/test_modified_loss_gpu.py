"""GPU tests of the modified (one symbol per frame) topology of the loss op (include/rnnt_modified.h compute_rnnt_loss_modified) against
the float64 restatement of tests/modified_cases.py.

Bars: the op's own fixed ones (include/rnnt.h) -- costs within 1e-4 max(1, |cost|), gradients within 1e-4 |cost_scale| absolute.
Padded cells and live cells outside the band (u <= t, L - u <= T - t) are exact zeros.  Every call through the C ABI gets a
gradient buffer and a workspace filled with 0xFF bytes (a backward-only call: the workspace its forward left).
The measured maxima are printed and, with MODIFIED_ACCURACY_DIR set, collected in modified_accuracy.json in that directory (kept
in profiles/modified_topology_notes.md)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib
from tests import fastemit_cases as fc
from tests import modified_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTOL = GTOL = 1e-4


def _record(route, **figures):
    row = {k: float(v) for k, v in figures.items()}
    print(route, row)
    out = os.environ.get("MODIFIED_ACCURACY_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "modified_accuracy.json")
    try:
        rows = json.load(open(path))
    except (OSError, ValueError):
        rows = {}
    rows[route] = row
    json.dump(rows, open(path, "w"), indent=1, sort_keys=True)


class ModCall:
    """The tensors of one call; the workspace and the gradient buffer start as 0xFF bytes."""

    def __init__(self, acts, labels, il, ll, blank=0, grad_offset_floats=0, stream=None):
        pkg.build()
        self.lib = _lib.load_mod()
        B, T, U, V = acts.shape
        self.shape = (B, T, U, V)
        d = torch.device(DEV)
        self.acts = torch.as_tensor(acts, device=d).contiguous()
        self.labels = torch.as_tensor(labels, device=d).contiguous()
        self.il = torch.as_tensor(il, device=d)
        self.ll = torch.as_tensor(ll, device=d)
        self.ws = torch.full((_lib.modified_workspace_bytes(T, U, B),), 0xFF, dtype=torch.uint8, device=d)
        self.costs = torch.full((B,), float("nan"), device=d)
        self.gbytes = torch.full(((acts.size + 8) * 4,), 0xFF, dtype=torch.uint8, device=d)
        self.grads = self.gbytes.view(torch.float32)[grad_offset_floats: grad_offset_floats + acts.size]
        self.blank = blank
        self.opts = _lib.make_options((stream or torch.cuda.current_stream()).cuda_stream, blank, T, U)

    def enqueue(self, lam=0.0, scale=None, costs=True, grads=True):
        B, T, U, V = self.shape
        return self.lib.compute_rnnt_loss_modified(
            self.acts.data_ptr(), self.grads.data_ptr() if grads else None, self.labels.data_ptr(), self.ll.data_ptr(),
            self.il.data_ptr(), scale.data_ptr() if scale is not None else None, V, B, self.costs.data_ptr() if costs else None,
            self.ws.data_ptr(), self.opts, lam)

    def run(self, lam=0.0, scale=None, costs=True, grads=True):
        """Poisons what the call is to write (the workspace too when the call runs the forward), runs it, returns (costs, grads)."""
        if grads:
            self.gbytes.fill_(0xFF)
        if costs:
            self.ws.fill_(0xFF)
            self.costs.fill_(float("nan"))
        scale_t = None if scale is None else torch.tensor(np.asarray(scale), dtype=torch.float32, device=DEV)
        assert self.enqueue(lam, scale_t, costs, grads) == 0
        return self.result()

    def result(self):
        torch.cuda.synchronize()
        return self.costs.cpu().numpy().astype(np.float64), self.grads.cpu().numpy().reshape(self.shape)


def _check(route, c, g, ref, il, ll, scale=None):
    """costs / gradients against the restatement `ref` with the fixed bars; exact zeros off the band; returns the maxima."""
    c_ref, g_ref = ref
    B = len(c_ref)
    cs = np.ones(B) if scale is None else np.abs(np.broadcast_to(np.asarray(scale, np.float64), (B,)))
    fin = np.isfinite(c_ref)
    assert np.array_equal(c[~fin], c_ref[~fin])  # an infeasible utterance: +inf exactly
    dc = np.abs(c[fin] - c_ref[fin]) / np.maximum(1.0, np.abs(c_ref[fin]))
    assert np.isfinite(g).all()
    dg = np.array([np.abs(g[b] - g_ref[b]).max() / max(cs[b], 1e-30) for b in range(B)])
    off = ~mc.band_mask(g.shape[:3], il, ll)
    zeros_ok = not g[off].any()
    _record(route, cost_rel=dc.max() if dc.size else 0.0, grad_abs_over_scale=dg.max())
    assert dc.size == 0 or dc.max() <= CTOL
    assert dg.max() <= GTOL
    assert zeros_ok
    return dc, dg


# ---- lane and wave edges ------------------------------------------------------------------------------------------------
EDGE_L = [62, 63, 64, 65, 127, 128, 129, 255, 256, 257]


def test_lane_and_wave_edges():
    """One utterance per width in ONE batch: the batch's maxU = 258 puts every utterance on the 6-columns-per-lane sweep, with its
    last column on, next to and across every multiple of 64 (the lane that owns L_b, the lane edge the label arrival crosses)."""
    B, V = len(EDGE_L), 5
    ll = np.array(EDGE_L, np.int32)
    il = ll + 3
    T, U = int(il.max()), int(ll.max()) + 1
    rng = np.random.default_rng(10)
    acts = rng.normal(size=(B, T, U, V)).astype(np.float32)
    labels = rng.integers(1, V, size=(B, U - 1)).astype(np.int32)
    k = ModCall(acts, labels, il, ll)
    c, g = k.run()
    _check("edges_B10_V5", c, g, mc.loss_and_grad(acts, labels, il, ll), il, ll)


@pytest.mark.parametrize("L", EDGE_L)
def test_lane_and_wave_edges_own_width(L):
    """The same widths with maxU = L + 1: each on the sweep its own width selects (1, 2, 3, 4 and 6 columns per lane)."""
    acts, labels, il, ll = mc.full_case(1, L + 3, L, 5, seed=L)
    k = ModCall(acts, labels, il, ll)
    c, g = k.run()
    _check(f"edge_L{L}_V5", c, g, mc.loss_and_grad(acts, labels, il, ll), il, ll)


# ---- ragged batch -------------------------------------------------------------------------------------------------------
def test_ragged_batch_with_an_infeasible_utterance():
    acts, labels, il, ll = mc.ragged_case()
    k = ModCall(acts, labels, il, ll)
    c, g = k.run()
    assert c[5] == np.inf and not g[5].any()  # (T, L) = (7, 12): no path -- +inf and zeros, never NaN
    _check("ragged_B6_T40_U21_V28", c, g, mc.loss_and_grad(acts, labels, il, ll), il, ll)
    # its neighbours do not see it: the same batch with that utterance made feasible gives them the same bits
    il2, ll2 = il.copy(), ll.copy()
    il2[5], ll2[5] = 12, 7
    c2, g2 = ModCall(acts, labels, il2, ll2).run()
    assert np.array_equal(c2[:5], c[:5]) and np.array_equal(g2[:5], g[:5]) and np.isfinite(c2[5])


# ---- vocabulary routes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [2, 3, 28, 29, 31, 60, 61, 64, 65, 128, 1024])
def test_vocabulary_routes(V):
    for blank in (0, V - 1, V // 2):
        acts, labels, il, ll = mc.full_case(2, 12, 5, V, seed=V, blank=blank)
        il[1], ll[1] = 9, 3
        assert not (labels == blank).any()
        k = ModCall(acts, labels, il, ll, blank=blank)
        c, g = k.run(lam=0.01)
        _check(f"vocab_V{V}_blank{blank}", c, g, mc.loss_and_grad(acts, labels, il, ll, 0.01, blank=blank), il, ll)


def test_unaligned_gradient_buffer():
    """V = 28 with a gradient buffer that is 4-byte aligned only: the scalar-store route."""
    acts, labels, il, ll = mc.full_case(2, 12, 5, 28, seed=7)
    k = ModCall(acts, labels, il, ll, grad_offset_floats=1)
    c, g = k.run()
    _check("unaligned_grads_V28", c, g, mc.loss_and_grad(acts, labels, il, ll), il, ll)


# ---- long paths ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_case(kind):
    if kind == "trained":
        case = fc.trained_like_case(2, 600, 151, 28, seed=21)
    else:
        case = fc.op_case(2, 600, 151, 28, seed=20, sigma={"n01": 1.0, "n08": 8.0}[kind])
    acts, labels, il, ll = case
    return case, mc.loss_and_grad(acts, labels, il, ll)


@pytest.mark.parametrize("kind", ["n01", "n08", "trained"])
def test_long_paths(kind):
    (acts, labels, il, ll), ref = _long_case(kind)
    c, g = ModCall(acts, labels, il, ll).run()
    _check(f"long_B2_T600_L150_V28_{kind}", c, g, ref, il, ll)


def test_wide_lattice():
    """More than 1024 columns: the 1024-thread sweep, columns crossing waves through LDS."""
    acts, labels, il, ll = mc.full_case(1, 1110, 1100, 4, seed=30)
    c, g = ModCall(acts, labels, il, ll).run()
    _check("wide_B1_T1110_L1100_V4", c, g, mc.loss_and_grad(acts, labels, il, ll), il, ll)


# ---- scaling and FastEmit -----------------------------------------------------------------------------------------------
def test_cost_scale_and_fastemit():
    acts, labels, il, ll = fc.op_case(3, 9, 5, 28, seed=40)
    B = 3
    k = ModCall(acts, labels, il, ll)
    c_first = None
    for sname, scale in (("null", None), ("mixed", np.array([-2.0, 0.5, 3.0])), ("mean", np.full(B, 1.0 / B))):
        for lam in (0.0, 0.01, 1.0):
            c, g = k.run(lam=lam, scale=scale)
            c_first = c if c_first is None else c_first
            assert np.array_equal(c, c_first)  # the costs depend neither on lambda nor on the scale, bit for bit
            _check(f"scale_{sname}_lambda{lam}", c, g, mc.loss_and_grad(acts, labels, il, ll, lam, scale), il, ll, scale)
    g0, g1 = k.run(lam=0.0)[1], k.run(lam=1.0)[1]
    assert np.abs(g1 - g0).max() > 1e-2  # lambda did something


# ---- calling conventions ------------------------------------------------------------------------------------------------
def test_split_calls_are_the_combined_call():
    acts, labels, il, ll = fc.op_case(3, 20, 9, 28, seed=50)
    scale = np.array([0.5, -1.0, 2.0])
    k = ModCall(acts, labels, il, ll)
    c, g = k.run(lam=0.25, scale=scale)
    cf, _ = k.run(lam=0.25, grads=False)                 # forward alone (poisoned workspace)
    assert np.array_equal(cf, c)
    _, gb = k.run(lam=0.25, scale=scale, costs=False)    # gradient pass alone, from the workspace that forward left
    assert np.array_equal(gb, g)
    _, gb2 = k.run(lam=0.25, scale=scale, costs=False)   # and once more
    assert np.array_equal(gb2, g)
    assert np.array_equal(k.result()[0], c)              # the gradient pass does not touch the costs


def test_graph_replay_is_the_direct_call():
    acts, labels, il, ll = fc.op_case(3, 20, 9, 28, seed=51)
    scale = torch.tensor([0.5, -1.0, 2.0], dtype=torch.float32, device=DEV)
    c, g = ModCall(acts, labels, il, ll).run(lam=0.25, scale=scale.cpu().numpy())
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):  # first use outside the capture
        k = ModCall(acts, labels, il, ll, stream=side)
        assert k.enqueue(0.25, scale) == 0
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        k.opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, *k.shape[1:3])
        assert k.enqueue(0.25, scale) == 0
    for _ in range(2):
        k.ws.fill_(0xFF)
        k.gbytes.fill_(0xFF)
        k.costs.fill_(float("nan"))
        graph.replay()
        cr, gr = k.result()
        assert np.array_equal(cr, c) and np.array_equal(gr, g)


# ---- out-of-range lengths -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,value", [("T", 0), ("T", 13), ("L", -1), ("L", 6)])
def test_out_of_range_lengths(what, value):
    """maxT = 12, maxU = 6: T_b in {0, maxT + 1}, L_b in {-1, maxU}.  That utterance is NaN, its neighbours are not touched."""
    acts, labels, il, ll = mc.full_case(3, 12, 5, 28, seed=60)
    il[0], ll[0] = 9, 3
    il_bad, ll_bad = il.copy(), ll.copy()
    (il_bad if what == "T" else ll_bad)[1] = value
    c, g = ModCall(acts, labels, il_bad, ll_bad).run(lam=0.01)
    assert np.isnan(c[1])
    Tc, Lc = min(max(int(il_bad[1]), 1), 12), min(max(int(ll_bad[1]), 0), 5)  # clamped into the tensor
    assert np.isnan(g[1, :Tc, : Lc + 1]).all()
    assert not g[1, Tc:].any() and not g[1, :, Lc + 1:].any()
    ref = mc.loss_and_grad(acts, labels, il, ll, 0.01)
    keep = [0, 2]
    _check(f"bad_{what}{value}", c[keep], g[keep], (ref[0][keep], ref[1][keep]), il[keep], ll[keep])
    c2, _ = ModCall(acts, labels, il, ll).run(lam=0.01)  # the process goes on
    assert np.isfinite(c2).all()


# ---- the Python surface -------------------------------------------------------------------------------------------------
def _torch_case(acts, labels, il, ll):
    x = torch.tensor(acts, device=DEV, requires_grad=True)
    return x, torch.tensor(labels, device=DEV), torch.tensor(il, device=DEV), torch.tensor(ll, device=DEV)


def test_autograd():
    pkg.build()
    acts, labels, il, ll = fc.op_case(3, 9, 5, 28, seed=70)
    w = np.array([0.5, -1.5, 2.0])
    x, y, t_il, t_ll = _torch_case(acts, labels, il, ll)
    costs = pkg.rnnt_loss(x, y, t_il, t_ll, fastemit_lambda=0.01, topology="modified")
    (torch.tensor(w, dtype=torch.float32, device=DEV) * costs).sum().backward()
    torch.cuda.synchronize()
    _check("autograd_weighted", costs.detach().cpu().numpy().astype(np.float64), x.grad.cpu().numpy(),
           mc.loss_and_grad(acts, labels, il, ll, 0.01, w), il, ll, w)
    # the module, mean reduction
    x, y, t_il, t_ll = _torch_case(acts, labels, il, ll)
    loss = pkg.RNNTLoss(reduction="mean", topology="modified")(x, y, t_il, t_ll)
    loss.backward()
    torch.cuda.synchronize()
    c_ref, g_ref = mc.loss_and_grad(acts, labels, il, ll, 0.0, 1.0 / 3)
    assert abs(float(loss.detach()) - c_ref.mean()) <= CTOL * max(1.0, abs(c_ref.mean()))
    _check("autograd_mean", c_ref, x.grad.cpu().numpy(), (c_ref, g_ref), il, ll, 1.0 / 3)
    # one call, no graph
    c1, g1 = pkg.rnnt_loss_and_grad(torch.tensor(acts, device=DEV), y, t_il, t_ll, fastemit_lambda=0.01, topology="modified")
    torch.cuda.synchronize()
    _check("loss_and_grad", c1.cpu().numpy().astype(np.float64), g1.cpu().numpy(), mc.loss_and_grad(acts, labels, il, ll, 0.01), il, ll)
    # get_loss_fn: lengths before the time reduction
    fn = pkg.get_loss_fn(2, topology="modified")
    c2 = fn(y, torch.tensor(acts, device=DEV), 2 * t_il, t_ll)
    assert np.array_equal(c2.cpu().numpy(), c1.cpu().numpy())


def test_standard_route_is_untouched():
    pkg.build()
    acts, labels, il, ll = fc.op_case(2, 12, 6, 28, seed=80)
    out = []
    for kw in ({}, {"topology": "standard"}):
        x, y, t_il, t_ll = _torch_case(acts, labels, il, ll)
        costs = pkg.rnnt_loss(x, y, t_il, t_ll, **kw)
        costs.sum().backward()
        torch.cuda.synchronize()
        out.append((costs.detach().cpu().numpy(), x.grad.cpu().numpy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    ca, ga = pkg.rnnt_loss_and_grad(torch.tensor(acts, device=DEV), *_torch_case(acts, labels, il, ll)[1:])
    cb, gb = pkg.rnnt_loss_and_grad(torch.tensor(acts, device=DEV), *_torch_case(acts, labels, il, ll)[1:], topology="standard")
    torch.cuda.synchronize()
    assert np.array_equal(ca.cpu().numpy(), cb.cpu().numpy()) and np.array_equal(ga.cpu().numpy(), gb.cpu().numpy())
    # and the modified lattice is another lattice
    cm = pkg.rnnt_loss(torch.tensor(acts, device=DEV), *_torch_case(acts, labels, il, ll)[1:], topology="modified")
    assert (np.abs(cm.cpu().numpy() - out[0][0]) > 1e-2).all()
