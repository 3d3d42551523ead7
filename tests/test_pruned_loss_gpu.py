"""GPU tests of the pruned transducer loss (include/rnnt_pruned.h compute_rnnt_loss_pruned) against the float64 restatement of
tests/pruned_cases.py, on both topologies.

Bars: the op's own fixed ones (include/rnnt.h) -- costs within 1e-4 max(1, |cost|), gradients within 1e-4 |cost_scale| absolute.
Every absent element of grads is an exact zero.  Every call through the C ABI gets a gradient buffer and a workspace filled with
0xFF bytes (a backward-only call: the workspace its forward left), and the logits of absent cells are NaN.
The measured maxima are printed and, with PRUNED_ACCURACY_DIR set, collected in pruned_accuracy.json in that directory (kept in
profiles/pruned_loss_notes.md)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib
from tests import fastemit_cases as fc
from tests import pruned_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTOL = GTOL = 1e-4
TOPO_ID = {"standard": 0, "modified": 1}
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -(2 ** 31)


def _record(route, **figures):
    row = {k: float(v) for k, v in figures.items()}
    print(route, row)
    out = os.environ.get("PRUNED_ACCURACY_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "pruned_accuracy.json")
    try:
        rows = json.load(open(path))
    except (OSError, ValueError):
        rows = {}
    rows[route] = row
    json.dump(rows, open(path, "w"), indent=1, sort_keys=True)


class PrunedCall:
    """The tensors of one call; the workspace and the gradient buffer start as 0xFF bytes."""

    def __init__(self, acts, sb, labels, il, ll, topology, blank=0, stream=None):
        pkg.build()
        self.lib = _lib.load_pruned()
        B, T, S, V = acts.shape
        self.shape = (B, T, S, V)
        self.maxU = labels.shape[1] + 1
        d = torch.device(DEV)
        self.acts = torch.as_tensor(acts, device=d).contiguous()
        self.sb = torch.as_tensor(np.asarray(sb, np.int32), device=d).contiguous()
        self.labels = torch.as_tensor(labels, device=d).contiguous()
        self.il = torch.as_tensor(il, device=d)
        self.ll = torch.as_tensor(ll, device=d)
        self.ws = torch.full((_lib.pruned_workspace_bytes(T, S, B),), 0xFF, dtype=torch.uint8, device=d)
        self.costs = torch.full((B,), float("nan"), device=d)
        self.gbytes = torch.full((acts.size * 4,), 0xFF, dtype=torch.uint8, device=d)
        self.grads = self.gbytes.view(torch.float32)
        self.topo = TOPO_ID[topology]
        self.blank = blank
        self.opts = _lib.make_options((stream or torch.cuda.current_stream()).cuda_stream, blank, T, self.maxU)

    def enqueue(self, lam=0.0, scale=None, costs=True, grads=True):
        B, T, S, V = self.shape
        return self.lib.compute_rnnt_loss_pruned(
            self.acts.data_ptr(), self.grads.data_ptr() if grads else None, self.sb.data_ptr(), self.labels.data_ptr(),
            self.ll.data_ptr(), self.il.data_ptr(), scale.data_ptr() if scale is not None else None, V, B, S, self.topo,
            self.costs.data_ptr() if costs else None, self.ws.data_ptr(), self.opts, lam)

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


def _check(route, c, g, ref, sb, il, ll, scale=None):
    """costs / gradients against the restatement `ref` with the fixed bars; exact zeros in absent cells; returns the maxima."""
    c_ref, g_ref = ref
    B = len(c_ref)
    cs = np.ones(B) if scale is None else np.abs(np.broadcast_to(np.asarray(scale, np.float64), (B,)))
    fin = np.isfinite(c_ref)
    assert np.array_equal(c[~fin], c_ref[~fin])  # a band that does not connect: +inf exactly
    dc = np.abs(c[fin] - c_ref[fin]) / np.maximum(1.0, np.abs(c_ref[fin]))
    assert np.isfinite(g).all()
    dg = np.array([np.abs(g[b] - g_ref[b]).max() / max(cs[b], 1e-30) for b in range(B)])
    zeros_ok = not g[~pc.present_mask(sb, il, ll, g.shape[2])].any() and not g[~fin].any()
    _record(route, cost_rel=dc.max() if dc.size else 0.0, grad_abs_over_scale=dg.max())
    assert dc.size == 0 or dc.max() <= CTOL
    assert dg.max() <= GTOL
    assert zeros_ok
    return dc, dg


def _run_case(route, case, topology, lam=0.0, blank=0):
    acts, sb, labels, il, ll = case
    c, g = PrunedCall(acts, sb, labels, il, ll, topology, blank=blank).run(lam=lam)
    ref = pc.loss_and_grad(acts, sb, labels, il, ll, lam=lam, blank=blank, topology=topology)
    _check(f"{route}_{topology}", c, g, ref, sb, il, ll)
    return c, g, ref


# ---- 1. lane-group edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pc.TOPOLOGIES)
@pytest.mark.parametrize("S", [1, 2, 3, 5, 8, 33, 64])
def test_lane_group_edges(S, topology):
    """B = 7: with 64 / G utterances per wavefront (G = the next power of two >= S) the last packed wavefront is partial for every
    S <= 32.  Utterance 0 (full length, L = 2 S + 2) takes steps of 0, 1 and S - 1: the standard lattice connects through them; the
    modified one cannot follow a step of S - 1 at frame 3 once S - 1 > 3 (a path has u <= t), which is legitimate data: +inf
    and zeros.  The others are ragged with L_b <= T_b - 2 on a straight line of steps 0 and 1, which connects on both lattices
    (S = 1 on the standard one: only without labels); utterance 2 has no labels."""
    acts, _, labels, il, ll = pc.band_case(7, 24, 2 * S + 2, S, 28, seed=100 + S)
    ll[1:] = np.minimum(ll[1:], il[1:] - 2)
    ll[2] = 0
    sb = np.zeros((7, 24), np.int32)
    seq = [0, 1, S - 1] + [1, 0] * 12  # utterance 0: the steps out of frames 0, 1, 2, ..., capped at the band's last position
    sb[0, 1:] = np.minimum(np.cumsum(seq[:23]), 2 * S + 3 - S)
    sb[0, 23] = 2 * S + 3 - S
    for b in range(1, 7):
        Tb, hi = int(il[b]), max(0, int(ll[b]) + 1 - S)
        sb[b] = np.minimum((np.arange(24) * hi) // max(Tb - 1, 1), hi)
    acts = pc.poison_absent(np.nan_to_num(acts), sb, il, ll)
    steps = np.diff(sb[0])
    assert {0, 1, S - 1} <= set(steps.tolist()) and set(np.diff(sb[1:, :12]).ravel().tolist()) <= {0, 1}
    c, _, ref = _run_case(f"lanes_S{S}", (acts, sb, labels, il, ll), topology)
    want = np.ones(7, bool)  # which utterances connect, by the reasoning above
    if S == 1 and topology == "standard":
        want = ll == 0
    if topology == "modified" and S - 1 > 3:
        want[0] = False
    assert np.array_equal(np.isfinite(ref[0]), want) and np.array_equal(np.isfinite(c), want)


# ---- 2. vocabularies ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pc.TOPOLOGIES)
@pytest.mark.parametrize("V", [2, 28, 29, 31, 1024])
def test_vocabularies(V, topology):
    for blank in (0, V // 2, V - 1):
        case = pc.band_case(3, 12, 8, 5, V, seed=V + blank, blank=blank, steps=[0, 1])
        assert not (case[2] == blank).any()
        c, _, _ = _run_case(f"vocab_V{V}_blank{blank}", case, topology, lam=0.01, blank=blank)
        assert np.isfinite(c[0])  # (a ragged utterance may have L_b > T_b: no path on the modified lattice, checked as such)


# ---- 3. hostile ranges --------------------------------------------------------------------------------------------------
def _hostile_case():
    B, T, S, V, L = 10, 10, 4, 28, 7
    rng = np.random.default_rng(300)
    labels = rng.integers(1, V, size=(B, L)).astype(np.int32)
    il, ll = np.full(B, T, np.int32), np.full(B, L, np.int32)
    good = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4], np.int32)
    sb = np.tile(good, (B, 1))
    sb[0] = [0, 0, 0, 4, 4, 4, 4, 4, 4, 4]           # a step of S: the bands do not touch
    sb[1] = [0, 1, 2, 1, 2, 3, 2, 3, 4, 4]           # decreasing in places
    sb[2] = [-2, -1, 0, 1, 1, 2, 2, 3, 4, 4]         # negative: cell (0, 0) sits at slot 2
    sb[3] = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]           # past L: the last rows have fewer and fewer present cells, then none
    sb[4] = [0, 1, 1, INT32_MAX, 2, 3, INT32_MIN, 4, 4, 4]
    ll[5] = 1                                        # L_b < S - 1
    sb[5] = 0
    il[6], ll[6] = 1, 0                              # T_b = 1
    sb[6] = 0
    ll[7] = 0                                        # L_b = 0
    sb[7] = [0, -1, -3, 0, 0, -2, 0, 0, -3, 0]
    il[8], ll[8] = 3, 6                              # L_b > T_b: no path on the modified lattice
    sb[8] = [0, 2, 3, 3, 3, 3, 3, 3, 3, 3]
    il[9], ll[9] = 1, 1                              # T_b = 1 with a label: the modified lattice's last frame emits it
    sb[9] = 0
    acts = rng.normal(size=(B, T, S, V)).astype(np.float32)
    return pc.poison_absent(acts, sb, il, ll), sb, labels, il, ll


@pytest.mark.parametrize("topology", pc.TOPOLOGIES)
def test_hostile_ranges(topology):
    case = _hostile_case()
    c, g, ref = _run_case("hostile", case, topology, lam=0.01)
    assert c[0] == np.inf and c[3] == np.inf and c[4] == np.inf and not g[[0, 3, 4]].any()
    assert np.isfinite(c[[1, 2, 5, 6, 7, 9]]).all()
    assert (c[8] == np.inf) == (topology == "modified")


# ---- 4. against the existing ops ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pc.TOPOLOGIES)
def test_the_full_band_is_the_existing_op(topology):
    acts, labels, il, ll = fc.op_case(4, 40, 21, 28, seed=400)
    sb = np.zeros((4, 40), np.int32)
    c, g, ref = _run_case("fullband_B4_T40_U21_V28", (acts, sb, labels, il, ll), topology, lam=0.01)
    t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    c2, g2 = pkg.rnnt_loss_and_grad(t(acts), t(labels), t(il), t(ll), fastemit_lambda=0.01, topology=topology)
    torch.cuda.synchronize()
    c2, g2 = c2.cpu().numpy().astype(np.float64), g2.cpu().numpy()
    assert (np.abs(c2 - ref[0]) <= CTOL * np.maximum(1.0, np.abs(ref[0]))).all() and np.abs(g2 - ref[1]).max() <= GTOL
    assert (np.abs(c2 - c) <= 2 * CTOL * np.maximum(1.0, np.abs(ref[0]))).all() and np.abs(g2 - g).max() <= 2 * GTOL


# ---- 5. long paths ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_full(kind):
    if kind == "trained":
        return pc.trained_like_case(2, 600, 150, 28, seed=21)
    return fc.op_case(2, 600, 151, 28, seed=20, sigma={"n01": 1.0, "n08": 8.0}[kind])


@functools.lru_cache(maxsize=None)
def _long_case(kind, topology):
    full, labels, il, ll = _long_full(kind)
    occ = pc.full_occupancy(full, labels, il, ll, topology=topology)
    sb = pkg.prune_ranges(torch.as_tensor(occ), torch.as_tensor(il), torch.as_tensor(ll), 5).numpy()
    acts = pc.poison_absent(pc.gather_band(full, sb, 5), sb, il, ll)
    return (acts, sb, labels, il, ll), pc.loss_and_grad(acts, sb, labels, il, ll, topology=topology)


@pytest.mark.parametrize("topology", pc.TOPOLOGIES)
@pytest.mark.parametrize("kind", ["n01", "n08", "trained"])
def test_long_paths(kind, topology):
    (acts, sb, labels, il, ll), ref = _long_case(kind, topology)
    assert np.isfinite(ref[0]).all()
    c, g = PrunedCall(acts, sb, labels, il, ll, topology).run()
    _check(f"long_B2_T600_L150_S5_V28_{kind}_{topology}", c, g, ref, sb, il, ll)


# ---- 6. scaling and FastEmit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pc.TOPOLOGIES)
def test_cost_scale_and_fastemit(topology):
    acts, sb, labels, il, ll = pc.band_case(3, 9, 5, 3, 28, seed=600, steps=[0, 1])
    B = 3
    k = PrunedCall(acts, sb, labels, il, ll, topology)
    c_first = None
    for sname, scale in (("null", None), ("mixed", np.array([-2.0, 0.5, 3.0])), ("mean", np.full(B, 1.0 / B))):
        for lam in (0.0, 0.01, 1.0):
            c, g = k.run(lam=lam, scale=scale)
            c_first = c if c_first is None else c_first
            assert np.array_equal(c, c_first)  # the costs depend neither on lambda nor on the scale, bit for bit
            ref = pc.loss_and_grad(acts, sb, labels, il, ll, lam, scale, topology=topology)
            _check(f"scale_{sname}_lambda{lam}_{topology}", c, g, ref, sb, il, ll, scale)
    assert np.isfinite(c_first).all()
    g0, g1 = k.run(lam=0.0)[1], k.run(lam=1.0)[1]
    assert np.abs(g1 - g0).max() > 1e-2  # lambda did something


# ---- 8. calling conventions ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pc.TOPOLOGIES)
def test_split_and_replayed_calls_are_the_combined_call(topology):
    # (a step of S - 1 = 3 early on leaves the modified lattice, where a path has u <= t, without a path)
    acts, sb, labels, il, ll = pc.band_case(3, 20, 9, 4, 28, seed=800, steps=[0, 1, 3] if topology == "standard" else [0, 1])
    scale_np = np.array([0.5, -1.0, 2.0])
    scale = torch.tensor(scale_np, dtype=torch.float32, device=DEV)
    c, g = PrunedCall(acts, sb, labels, il, ll, topology).run(lam=0.25, scale=scale_np)
    assert np.isfinite(c).all()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):  # everything below on a stream of its own
        k = PrunedCall(acts, sb, labels, il, ll, topology, stream=side)
        cf, _ = k.run(lam=0.25, grads=False)                    # forward alone (poisoned workspace)
        assert np.array_equal(cf, c, equal_nan=True)
        _, gb = k.run(lam=0.25, scale=scale_np, costs=False)    # gradient pass alone, from the workspace that forward left
        assert np.array_equal(gb, g)
        _, gb2 = k.run(lam=0.25, scale=scale_np, costs=False)   # and once more
        assert np.array_equal(gb2, g)
        assert np.array_equal(k.result()[0], c)                 # the gradient pass does not touch the costs
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        k.opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, k.shape[1], k.maxU)
        assert k.enqueue(0.25, scale) == 0
    for _ in range(2):
        k.ws.fill_(0xFF)
        k.gbytes.fill_(0xFF)
        k.costs.fill_(float("nan"))
        graph.replay()
        cr, gr = k.result()
        assert np.array_equal(cr, c) and np.array_equal(gr, g)


# ---- out-of-range lengths -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,value", [("T", 0), ("T", 13), ("L", -1), ("L", 9)])
def test_out_of_range_lengths(what, value):
    """maxT = 12, maxU = 9: that utterance is NaN on the present cells of its clamped lattice, its neighbours are not touched."""
    acts, sb, labels, il, ll = pc.band_case(3, 12, 8, 5, 28, seed=900, ragged=False, steps=[0, 1])
    acts = np.nan_to_num(acts)
    il_bad, ll_bad = il.copy(), ll.copy()
    (il_bad if what == "T" else ll_bad)[1] = value
    c, g = PrunedCall(acts, sb, labels, il_bad, ll_bad, "standard").run(lam=0.01)
    assert np.isnan(c[1])
    il_c, ll_c = np.clip(il_bad, 1, 12), np.clip(ll_bad, 0, 8)
    m = pc.present_mask(sb, il_c, ll_c, 5)[1]
    assert np.isnan(g[1][m]).all() and not g[1][~m].any()
    ref = pc.loss_and_grad(acts, sb, labels, il, ll, 0.01)
    keep = [0, 2]
    _check(f"bad_{what}{value}", c[keep], g[keep], (ref[0][keep], ref[1][keep]), sb[keep], il[keep], ll[keep])


# ---- 9. autograd --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pc.TOPOLOGIES)
def test_autograd(topology):
    pkg.build()
    acts, sb, labels, il, ll = pc.band_case(3, 9, 5, 3, 28, seed=1000, steps=[0, 1])
    t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    c1, g1 = pkg.rnnt_loss_pruned_and_grad(t(acts), t(sb), t(labels), t(il), t(ll), fastemit_lambda=0.01, topology=topology)
    x = torch.tensor(acts, device=DEV, requires_grad=True)
    ranges = t(sb)[:, :, None] + torch.arange(3, device=DEV, dtype=torch.int32)  # k2's [B, T, S] form
    costs = pkg.rnnt_loss_pruned(x, ranges, t(labels), t(il), t(ll), fastemit_lambda=0.01, topology=topology)
    costs.sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(costs.detach(), c1) and torch.equal(x.grad, g1)
    ref = pc.loss_and_grad(acts, sb, labels, il, ll, 0.01, topology=topology)
    _check(f"autograd_{topology}", c1.cpu().numpy().astype(np.float64), g1.cpu().numpy(), ref, sb, il, ll)
    # weighted
    w = np.array([0.5, -1.5, 2.0])
    x = torch.tensor(acts, device=DEV, requires_grad=True)
    costs = pkg.rnnt_loss_pruned(x, t(sb), t(labels), t(il), t(ll), fastemit_lambda=0.01, topology=topology)
    (torch.tensor(w, dtype=torch.float32, device=DEV) * costs).sum().backward()
    torch.cuda.synchronize()
    _check(f"autograd_weighted_{topology}", costs.detach().cpu().numpy().astype(np.float64), x.grad.cpu().numpy(),
           pc.loss_and_grad(acts, sb, labels, il, ll, 0.01, w, topology=topology), sb, il, ll, w)


# ---- 10. end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pc.TOPOLOGIES)
def test_end_to_end(topology):
    """prune_ranges -> prune_joint_inputs -> a torch joint -> rnnt_loss_pruned: the gradients with respect to enc and pred equal
    those of the restatement chained through a float64 torch joint."""
    pkg.build()
    B, T, U, J, V, S = 2, 30, 12, 16, 12, 4
    enc, pred, _, _, W2, b2, labels, il, ll = fc.joint_case(B, T, U, J, J, V, seed=1100)
    full = np.tanh(enc[:, :, None, :].astype(np.float64) + pred[:, None, :, :]) @ W2.astype(np.float64) + b2
    occ = pc.full_occupancy(full, labels, il, ll, topology=topology)

    def forward(dev, dtype):
        e = torch.tensor(enc, device=dev, dtype=dtype, requires_grad=True)
        p = torch.tensor(pred, device=dev, dtype=dtype, requires_grad=True)
        t = lambda a: torch.as_tensor(a, device=dev)  # noqa: E731
        sb = pkg.prune_ranges(t(occ), t(il), t(ll), S)
        a, q = pkg.prune_joint_inputs(e, p, sb, S)
        logits = torch.tanh(a + q) @ t(W2).to(dtype) + t(b2).to(dtype)
        return e, p, sb, logits

    e, p, sb, logits = forward(DEV, torch.float32)
    t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    costs = pkg.rnnt_loss_pruned(logits, sb, t(labels), t(il), t(ll), topology=topology)
    costs.sum().backward()
    torch.cuda.synchronize()
    # the reference: the same chain in float64 on the CPU, the restatement's gradients pushed through the joint
    e64, p64, sb64, logits64 = forward("cpu", torch.float64)
    assert torch.equal(sb64, sb.cpu())
    c_ref, g_ref = pc.loss_and_grad(logits64.detach().numpy(), sb64.numpy(), labels, il, ll, topology=topology)
    logits64.backward(torch.as_tensor(g_ref))
    assert np.isfinite(c_ref).all()
    dc = np.abs(costs.detach().cpu().numpy() - c_ref) / np.maximum(1.0, np.abs(c_ref))
    de = (e.grad.cpu().double() - e64.grad).abs().max().item()
    dp = (p.grad.cpu().double() - p64.grad).abs().max().item()
    _record(f"end_to_end_{topology}", cost_rel=dc.max(), d_enc=de, d_pred=dp)
    assert dc.max() <= CTOL and de <= 1e-4 and dp <= 1e-4
    assert e64.grad.abs().max() > 1e-2 and p64.grad.abs().max() > 1e-2
