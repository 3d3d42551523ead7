"""GPU tests of the fused joint on the pruned band (include/rnnt_pruned_joint.h compute_rnnt_joint_loss_pruned) against the float64
restatement of tests/pruned_joint_cases.py, on both topologies.

Bars: the project's for the f32-grade fused joint (tests/test_joint_gpu.py) -- costs and every gradient tensor within
1e-4 max(1, max |reference|), gradients times |cost_scale|.  With M the largest |entry| of a gradient's reference at unit
cost_scale: an utterance's rows of d_enc_proj / d_pred_proj are within 1e-4 |cost_scale_b| max(1, M), and dW2 / db2 (sums over
the batch) within 1e-4 max |cost_scale| max(1, M); a cost within 1e-4 max(1, |cost|).  Rows of d_enc_proj / d_pred_proj no present
cell points at, and everything of an utterance whose band does not connect, are exact zeros.
Every call through the C ABI gets gradient buffers and a workspace filled with 0xFF bytes (a gradient-only call: the workspace its
forward left); the rows of enc_proj beyond T_b and of pred_proj beyond L_b are NaN; W2 and b2 sit, exactly to size, in front of
NaN: a column beyond V that was loaded and not masked would arrive in the results.
The measured maxima are printed and, with PRUNED_JOINT_ACCURACY_DIR set, collected in pruned_joint_accuracy.json in that directory
(kept in profiles/pruned_joint_notes.md)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib
from rnnt_speech_recognition_amd.joint import _JointLossFunction
from tests import pruned_joint_cases as pj

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
TOPO_ID = {"standard": 0, "modified": 1}
KEYS = pj.GRAD_KEYS


def _record(route, **figures):
    row = {k: float(v) for k, v in figures.items()}
    print(route, row)
    out = os.environ.get("PRUNED_JOINT_ACCURACY_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "pruned_joint_accuracy.json")
    try:
        rows = json.load(open(path))
    except (OSError, ValueError):
        rows = {}
    rows[route] = row
    json.dump(rows, open(path, "w"), indent=1, sort_keys=True)


def _exact(x, d):
    """x at the head of a buffer whose tail is NaN: the tensor ends where its data ends."""
    x = np.ascontiguousarray(x, np.float32)
    buf = torch.full((x.size + 4096,), float("nan"), device=d)
    buf[: x.size] = torch.as_tensor(x.ravel(), device=d)
    return buf[: x.size].view(*x.shape)


class JointCall:
    """The tensors of one call; the workspace and the gradient buffers start as 0xFF bytes."""

    def __init__(self, case, topology, blank=0, stream=None):
        pkg.build()
        self.lib = _lib.load_prunedjoint()
        d = torch.device(DEV)
        enc, pred = case["enc"], case["pred"]
        self.B, self.T, self.J = enc.shape
        self.U, self.V, self.S = pred.shape[1], case["W2"].shape[1], case["S"]
        self.enc = torch.as_tensor(enc, device=d).contiguous()
        self.pred = torch.as_tensor(pred, device=d).contiguous()
        self.W2, self.b2 = _exact(case["W2"], d), _exact(case["b2"], d)
        self.sb = torch.as_tensor(np.asarray(case["sb"], np.int32), device=d).contiguous()
        self.labels = torch.as_tensor(case["labels"], device=d).contiguous()
        self.il = torch.as_tensor(case["il"], device=d)
        self.ll = torch.as_tensor(case["ll"], device=d)
        assert self.labels.shape[1] == max(self.U - 1, 1)
        self.ws = torch.full((_lib.pruned_joint_workspace_bytes(self.T, self.S, self.B, self.J),), 0xFF, dtype=torch.uint8, device=d)
        self.costs = torch.full((self.B,), float("nan"), device=d)
        self.shapes = ((self.B, self.T, self.J), (self.B, self.U, self.J), (self.J, self.V), (self.V,))
        self.gbytes = [torch.full((int(np.prod(s)) * 4,), 0xFF, dtype=torch.uint8, device=d) for s in self.shapes]
        self.topo = TOPO_ID[topology]
        self.blank = blank
        self.opts = _lib.make_options((stream or torch.cuda.current_stream()).cuda_stream, blank, self.T, self.U)

    def enqueue(self, lam=0.0, scale=None, costs=True, grads=True):
        g = [b.data_ptr() if grads else None for b in self.gbytes]
        return self.lib.compute_rnnt_joint_loss_pruned(
            self.enc.data_ptr(), self.pred.data_ptr(), self.W2.data_ptr(), self.b2.data_ptr(), self.sb.data_ptr(),
            self.labels.data_ptr(), self.ll.data_ptr(), self.il.data_ptr(), scale.data_ptr() if scale is not None else None,
            self.J, self.V, self.B, self.S, self.topo, self.costs.data_ptr() if costs else None, g[0], g[1], g[2], g[3],
            self.ws.data_ptr(), self.opts, lam)

    def run(self, lam=0.0, scale=None, costs=True, grads=True):
        """Poisons what the call is to write (the workspace too when the call runs the forward), runs it, returns the results."""
        if grads:
            for b in self.gbytes:
                b.fill_(0xFF)
        if costs:
            self.ws.fill_(0xFF)
            self.costs.fill_(float("nan"))
        scale_t = None if scale is None else torch.tensor(np.asarray(scale), dtype=torch.float32, device=DEV)
        assert self.enqueue(lam, scale_t, costs, grads) == 0
        return self.result()

    def result(self):
        torch.cuda.synchronize()
        out = dict(costs=self.costs.cpu().numpy().astype(np.float64))
        for key, b, s in zip(KEYS, self.gbytes, self.shapes):
            out[key] = b.view(torch.float32).cpu().numpy().reshape(s)
        return out


def _ref(case, lam=0.0, scale=None, blank=0, topology="standard"):
    return pj.loss_and_grads(case["enc"], case["pred"], case["W2"], case["b2"], case["sb"], case["labels"], case["il"], case["ll"],
                             case["S"], lam, scale, blank, topology)


def _check(route, got, ref, case, scale=None, keep=None):
    """Costs and the four gradients against the restatement with the fixed bars; exact zeros where the contract has them.
    `keep`: the utterances to look at (the others are out of range: NaN, checked by the caller)."""
    B = len(ref["costs"])
    keep = np.arange(B) if keep is None else np.asarray(keep)
    cs = np.ones(B) if scale is None else np.abs(np.broadcast_to(np.asarray(scale, np.float64), (B,)))
    c, c_ref = got["costs"][keep], ref["costs"][keep]
    fin = np.isfinite(c_ref)
    assert np.array_equal(c[~fin], c_ref[~fin])  # a band that does not connect: +inf exactly
    dc = np.abs(c[fin] - c_ref[fin]) / np.maximum(1.0, np.abs(c_ref[fin]))
    figures = dict(cost_rel=dc.max() if dc.size else 0.0)
    worst = figures["cost_rel"] / TOL
    for key in ("d_enc", "d_pred"):
        assert np.isfinite(got[key][keep]).all(), key
        unit = max(1.0, max(np.abs(ref[key][b]).max() / cs[b] for b in keep if cs[b] > 0))  # max |reference| at unit scale
        r = max(np.abs(got[key][b] - ref[key][b]).max() / max(cs[b] * unit, 1e-30) for b in keep)
        figures[key] = r
        worst = max(worst, r / TOL)
    if len(keep) == B:
        for key in ("dW2", "db2"):
            assert np.isfinite(got[key]).all(), key
            r = np.abs(got[key] - ref[key]).max() / max(cs.max(), np.abs(ref[key]).max(), 1e-30)
            figures[key] = r
            worst = max(worst, r / TOL)
    _record(route, **figures)
    assert worst <= 1.0, figures
    rows_e, rows_p = pj.touched_rows(case["sb"], case["il"], case["ll"], case["S"], got["d_enc"].shape[1], got["d_pred"].shape[1])
    for b in keep:
        assert not got["d_enc"][b][~rows_e[b]].any() and not got["d_pred"][b][~rows_p[b]].any(), b
        if not np.isfinite(ref["costs"][b]):
            assert not got["d_enc"][b].any() and not got["d_pred"][b].any(), b
    return figures


def _run_case(route, case, topology, lam=0.0, blank=0, scale=None):
    got = JointCall(case, topology, blank=blank).run(lam=lam, scale=scale)
    ref = _ref(case, lam, scale, blank, topology)
    _check(f"{route}_{topology}", got, ref, case, scale)
    return got, ref


# ---- 1. vocabulary tile edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
@pytest.mark.parametrize("V", [2, 28, 31, 32, 33, 65, 129, 500])
def test_vocabulary_tile_edges(V, topology):
    for blank in (0, V // 2, V - 1):
        case = pj.joint_case(3, 12, 8, 5, 64, V, seed=V + blank, blank=blank, line=True)
        assert not (case["labels"] == blank).any()
        got, _ = _run_case(f"vocab_V{V}_blank{blank}", case, topology, lam=0.01, blank=blank)
        assert np.isfinite(got["costs"]).all()


# ---- 2. joint widths ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
@pytest.mark.parametrize("J", [64, 128, 320, 640])
def test_joint_widths(J, topology):
    case = pj.joint_case(3, 12, 8, 5, J, 33, seed=200 + J, line=True)
    got, _ = _run_case(f"width_J{J}", case, topology, lam=0.01)
    assert np.isfinite(got["costs"]).all()


# ---- 3. band widths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
@pytest.mark.parametrize("S", [1, 2, 3, 5, 8, 33, 64])
def test_band_widths(S, topology):
    """The ranges of tests/test_pruned_loss_gpu.py test_lane_group_edges (B7 T24 ragged, L = 2 S + 2: steps of 0, 1 and S - 1 in
    utterance 0, straight lines in the others, utterance 2 without labels): the lane-group edges of the sweep, and row tiles of 32
    slots that begin in the middle of a frame for every S that does not divide 32."""
    B, T, L = 7, 24, 2 * S + 2
    case = pj.joint_case(B, T, L, S, 64, 28, seed=300 + S)
    il, ll = case["il"], case["ll"]
    ll[1:] = np.minimum(ll[1:], il[1:] - 2)
    ll[2] = 0
    sb = pj.straight_ranges(T, S, il, ll)
    seq = [0, 1, S - 1] + [1, 0] * 12
    sb[0, 0] = 0
    sb[0, 1:] = np.minimum(np.cumsum(seq[:23]), 2 * S + 3 - S)
    sb[0, 23] = 2 * S + 3 - S
    case["sb"] = sb
    case["enc"], case["pred"] = pj.poison_rows(np.nan_to_num(case["enc"]), np.nan_to_num(case["pred"]), il, ll)
    got, ref = _run_case(f"band_S{S}", case, topology)
    want = np.ones(B, bool)  # which utterances connect (the reasoning of test_lane_group_edges)
    if S == 1 and topology == "standard":
        want = ll == 0
    if topology == "modified" and S - 1 > 3:
        want[0] = False
    assert np.array_equal(np.isfinite(ref["costs"]), want) and np.array_equal(np.isfinite(got["costs"]), want)


# ---- 4. hostile ranges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
def test_hostile_ranges(topology):
    case = pj.hostile_case()
    got, ref = _run_case("hostile", case, topology, lam=0.01)
    c = got["costs"]
    assert c[0] == np.inf and c[3] == np.inf and c[4] == np.inf
    assert np.isfinite(c[[1, 2, 5, 6, 7, 9]]).all()
    assert (c[8] == np.inf) == (topology == "modified")


@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
@pytest.mark.parametrize("what,value", [("T", 0), ("T", 13), ("L", -1), ("L", 9)])
def test_out_of_range_lengths(what, value, topology):
    """maxT = 12, maxU = 9: that utterance is NaN where its clamped lattice's present cells point, its neighbours are not touched."""
    case = pj.joint_case(3, 12, 8, 5, 64, 28, seed=900, ragged=False, line=True)
    good = _ref(case, 0.01, topology=topology)
    assert np.isfinite(good["costs"]).all()
    (case["il"] if what == "T" else case["ll"])[1] = value
    got = JointCall(case, topology).run(lam=0.01)
    assert np.isnan(got["costs"][1])
    rows_e, rows_p = pj.touched_rows(case["sb"], case["il"], case["ll"], 5, 12, 9)
    assert np.isnan(got["d_enc"][1][rows_e[1]]).all() and not got["d_enc"][1][~rows_e[1]].any()
    assert np.isnan(got["d_pred"][1][rows_p[1]]).all() and not got["d_pred"][1][~rows_p[1]].any()
    assert np.isnan(got["dW2"]).all() and np.isnan(got["db2"]).all()
    _check(f"bad_{what}{value}_{topology}", got, good, case, keep=[0, 2])


# ---- 5. the full band ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
def test_the_full_band_is_the_existing_routes(topology):
    """s_begin = 0, S = U: the fused joint of the full lattice (joint_dtype 0; standard lattice only) and the composed route
    (prune_joint_inputs -> torch joint -> rnnt_loss_pruned; both lattices) compute the same thing."""
    B, T, U, J, V = 4, 40, 21, 64, 28
    case = pj.joint_case(B, T, U - 1, U, J, V, seed=400)
    case["sb"] = np.zeros((B, T), np.int32)
    got, ref = _run_case("fullband_B4_T40_U21_J64_V28", case, topology, lam=0.01)
    assert np.isfinite(ref["costs"]).all()
    t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    leaves = lambda: [torch.tensor(np.nan_to_num(case[k]), device=DEV, requires_grad=True) for k in ("enc", "pred", "W2", "b2")]  # noqa: E731
    labels, il, ll = t(case["labels"]), t(case["il"]), t(case["ll"])

    def against(route, costs, xs):
        costs.sum().backward()
        torch.cuda.synchronize()
        other = dict(costs=costs.detach().cpu().numpy().astype(np.float64))
        other.update({k: x.grad.cpu().numpy() for k, x in zip(KEYS, xs)})
        _check(f"{route}_{topology}", other, ref, case)  # the other route against the restatement,
        for k in ("costs",) + KEYS:                      # and the two routes against each other, at the same bar
            assert np.abs(other[k] - got[k]).max() <= TOL * max(1.0, np.abs(ref[k]).max()), k

    xs = leaves()
    a, q = pkg.prune_joint_inputs(xs[0], xs[1], t(case["sb"]), U)
    against("fullband_composed", pkg.rnnt_loss_pruned(torch.tanh(a + q) @ xs[2] + xs[3], t(case["sb"]), labels, il, ll,
                                                      fastemit_lambda=0.01, topology=topology), xs)
    if topology == "standard":
        xs = leaves()
        against("fullband_joint_dtype0", _JointLossFunction.apply(*xs, labels, il, ll, 0, 0, 0.01), xs)


# ---- 6. magnitudes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
@pytest.mark.parametrize("kind", ["w2_1e-36", "w2_1e-3", "w2_1e3", "peaked"])
def test_magnitudes(kind, topology):
    """W2 a thousand times smaller / larger than glorot (the power-of-two scale of W2), W2 below 2^-113 (where the scale stops
    growing: nothing may overflow), and 8 x N(0,1) projections (saturated h)."""
    kw = {"w2_1e-36": dict(w_scale=1e-36), "w2_1e-3": dict(w_scale=1e-3), "w2_1e3": dict(w_scale=1e3), "peaked": dict(sigma=8.0)}[kind]
    case = pj.joint_case(3, 12, 8, 5, 128, 33, seed=600, line=True, **kw)
    got, _ = _run_case(f"magnitude_{kind}", case, topology)
    assert np.isfinite(got["costs"]).all()


# ---- 7. scaling and FastEmit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
def test_cost_scale_and_fastemit(topology):
    case = pj.joint_case(3, 9, 5, 3, 64, 28, seed=700, line=True)
    B = 3
    k = JointCall(case, topology)
    c_first = None
    for sname, scale in (("null", None), ("mixed", np.array([-2.0, 0.5, 3.0])), ("mean", np.full(B, 1.0 / B))):
        for lam in (0.0, 0.01, 1.0):
            got = k.run(lam=lam, scale=scale)
            c_first = got["costs"] if c_first is None else c_first
            assert np.array_equal(got["costs"], c_first)  # the costs depend neither on lambda nor on the scale, bit for bit
            _check(f"scale_{sname}_lambda{lam}_{topology}", got, _ref(case, lam, scale, topology=topology), case, scale)
    assert np.isfinite(c_first).all()
    g0, g1 = k.run(lam=0.0)["d_enc"], k.run(lam=1.0)["d_enc"]
    assert np.abs(g1 - g0).max() > 1e-3  # lambda did something


# ---- 8. calling conventions, bit for bit --------------------------------------------------------------------------------
def _same(x, y, keys=("costs",) + KEYS):
    return all(np.array_equal(x[k], y[k], equal_nan=True) for k in keys)


@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
def test_split_and_replayed_calls_are_the_combined_call(topology):
    # (a step of S - 1 = 3 early on leaves the modified lattice, where a path has u <= t, without a path: a straight line there)
    # J = 640: the tile kernels take more than 64 KB of LDS, asked for in front of every launch, under stream capture too
    case = pj.joint_case(3, 20, 9, 4, 640, 33, seed=800, steps=[0, 1, 3], line=topology == "modified")
    scale_np = np.array([0.5, -1.0, 2.0])
    scale = torch.tensor(scale_np, dtype=torch.float32, device=DEV)
    k0 = JointCall(case, topology)
    want = k0.run(lam=0.25, scale=scale_np)
    assert np.isfinite(want["costs"]).all()
    assert _same(k0.run(lam=0.25, scale=scale_np), want)           # a second identical call
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):  # everything below on a stream of its own
        k = JointCall(case, topology, stream=side)
        assert np.array_equal(k.run(lam=0.25, grads=False)["costs"], want["costs"])  # forward alone (poisoned workspace)
        assert _same(k.run(lam=0.25, scale=scale_np, costs=False), want)             # gradient pass alone, from that workspace
        assert _same(k.run(lam=0.25, scale=scale_np, costs=False), want)             # and once more
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        k.opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, k.T, k.U)
        assert k.enqueue(0.25, scale) == 0
    for _ in range(2):
        k.ws.fill_(0xFF)
        for b in k.gbytes:
            b.fill_(0xFF)
        k.costs.fill_(float("nan"))
        graph.replay()
        assert _same(k.result(), want)


@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
def test_an_utterance_alone_is_the_utterance_in_a_batch(topology):
    case = pj.joint_case(4, 14, 7, 3, 64, 31, seed=810, line=True)
    scale = np.array([0.5, -1.0, 2.0, 0.25])
    batch = JointCall(case, topology).run(lam=0.01, scale=scale)
    for b in (1, 3):
        one = {k: (v[b:b + 1] if k not in ("W2", "b2", "S") else v) for k, v in case.items()}
        alone = JointCall(one, topology).run(lam=0.01, scale=scale[b:b + 1])
        for key in ("costs", "d_enc", "d_pred"):
            assert np.array_equal(alone[key][0], batch[key][b], equal_nan=True), (b, key)


# ---- 9. autograd and the two-pass pipeline ------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
def test_autograd(topology):
    pkg.build()
    case = pj.joint_case(3, 9, 5, 3, 64, 28, seed=1000, line=True)
    t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    rest = (t(case["labels"]), t(case["il"]), t(case["ll"]))
    one = pkg.rnnt_joint_loss_pruned_and_grad(t(case["enc"]), t(case["pred"]), t(case["W2"]), t(case["b2"]), t(case["sb"]), *rest,
                                              fastemit_lambda=0.01, topology=topology, s_range=3)
    xs = [torch.tensor(case[k], device=DEV, requires_grad=True) for k in ("enc", "pred", "W2", "b2")]
    ranges = t(case["sb"])[:, :, None] + torch.arange(3, device=DEV, dtype=torch.int32)  # k2's [B, T, S] form
    costs = pkg.rnnt_joint_loss_pruned(*xs, ranges, *rest, fastemit_lambda=0.01, topology=topology)
    costs.sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(costs.detach(), one[0])
    # (the combined call has cost_scale NULL, autograd hands in ones: the same products)
    got = dict(costs=costs.detach().cpu().numpy().astype(np.float64), **{k: x.grad.cpu().numpy() for k, x in zip(KEYS, xs)})
    for k, g in zip(KEYS, one[1:]):
        assert np.array_equal(got[k], g.cpu().numpy()), k
    _check(f"autograd_{topology}", got, _ref(case, 0.01, topology=topology), case)
    w = np.array([0.5, -1.5, 2.0])
    xs = [torch.tensor(case[k], device=DEV, requires_grad=True) for k in ("enc", "pred", "W2", "b2")]
    costs = pkg.rnnt_joint_loss_pruned(*xs, t(case["sb"]), *rest, fastemit_lambda=0.01, topology=topology, s_range=3)
    (torch.tensor(w, dtype=torch.float32, device=DEV) * costs).sum().backward()
    torch.cuda.synchronize()
    got = dict(costs=costs.detach().cpu().numpy().astype(np.float64), **{k: x.grad.cpu().numpy() for k, x in zip(KEYS, xs)})
    _check(f"autograd_weighted_{topology}", got, _ref(case, 0.01, w, topology=topology), case, w)


@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
def test_two_pass_fused_is_two_pass_with_the_torch_joint(topology):
    """B2 T30 U12 J64 V12 S4 on the device: the same bands; costs and gradients of the two routes within the bar of each other,
    and each within the bar of the float64 restatement on those bands."""
    pkg.build()
    B, T, U, J, V, S = 2, 30, 12, 64, 12, 4
    rng = np.random.default_rng(1100)
    mk = lambda *shape: rng.normal(size=shape).astype(np.float32)  # noqa: E731
    am, lm, enc, pred = mk(B, T, V), mk(B, U, V), mk(B, T, J), mk(B, U, J)
    W2, b2 = (0.3 * mk(J, V)).astype(np.float32), (0.1 * mk(V)).astype(np.float32)
    labels = rng.integers(1, V, size=(B, U - 1)).astype(np.int32)
    il, ll = np.array([T, T - 4], np.int32), np.array([U - 1, U - 3], np.int32)
    t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731

    def run(fused):
        xs = [torch.tensor(a, device=DEV, requires_grad=True) for a in (am, lm, enc, pred, W2, b2)]
        a, l, e, p, W, bias = xs
        if fused:
            sc, pcost, sb = pkg.rnnt_loss_two_pass_fused(a, l, e, p, W, bias, t(labels), t(il), t(ll), S, fastemit_lambda=0.01,
                                                         topology=topology)
        else:
            sc, pcost, sb = pkg.rnnt_loss_two_pass(a, l, e, p, lambda x, y: torch.tanh(x + y) @ W + bias, t(labels), t(il), t(ll), S,
                                                   fastemit_lambda=0.01, topology=topology)
        (0.5 * sc.sum() + pcost.sum()).backward()
        torch.cuda.synchronize()
        out = dict(costs=pcost.detach().cpu().numpy().astype(np.float64), **{k: x.grad.cpu().numpy() for k, x in zip(KEYS, xs[2:])})
        return sc.detach().cpu(), sb.cpu().numpy(), out, [xs[0].grad.cpu(), xs[1].grad.cpu()]

    s1, sb1, g1, first1 = run(True)
    s0, sb0, g0, first0 = run(False)
    assert np.array_equal(sb1, sb0) and torch.equal(s1, s0) and all(torch.equal(x, y) for x, y in zip(first1, first0))
    case = dict(enc=enc, pred=pred, W2=W2, b2=b2, sb=sb1, labels=labels, il=il, ll=ll, S=S)
    ref = _ref(case, 0.01, topology=topology)
    assert np.isfinite(ref["costs"]).all()
    _check(f"two_pass_fused_{topology}", g1, ref, case)
    _check(f"two_pass_composed_{topology}", g0, ref, case)
    for k in ("costs",) + KEYS:
        assert np.abs(g1[k] - g0[k]).max() <= TOL * max(1.0, np.abs(ref[k]).max()), k
    assert np.abs(g1["d_enc"]).max() > 1e-2 and np.abs(g1["dW2"]).max() > 1e-2


# ---- 10. long sweeps ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_case():
    return pj.joint_case(2, 600, 150, 5, 128, 28, seed=1200, line=True)


@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
def test_long_sweeps(topology):
    """B2 T600 L150 S5 J128 V28: 94 row tiles per utterance, two row chunks or more in the dW2 pass."""
    case = _long_case()
    got, ref = _run_case("long_B2_T600_L150_S5_J128_V28", case, topology)
    assert np.isfinite(ref["costs"]).all()
