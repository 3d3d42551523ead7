"""GPU tests of the simple (additive joiner) transducer loss (include/rnnt_simple.h compute_rnnt_loss_simple) against the float64
restatement of tests/simple_cases.py, on both topologies.

Bars, the project's fixed ones: costs within 1e-4 max(1, |cost|), occupancy within 1e-4 absolute, grad_am and grad_lm within
1e-4 |cost_scale| max(1, max |reference|) per utterance (the fused joints' bar: they are sums over cells).  Exact zeros on absent
cells and padded rows, +inf / NaN exactly where the contract says so.  Every call through the C ABI gets a workspace and outputs
filled with 0xFF bytes (a gradient-only call: the workspace its forward left), and the input rows the op must not read are NaN.
The measured maxima are printed and, with SIMPLE_ACCURACY_DIR set, collected in simple_accuracy.json in that directory (kept in
profiles/simple_loss_notes.md)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib
from tests import fastemit_cases as fc
from tests import simple_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTOL = OTOL = GTOL = 1e-4
TOPO_ID = {"standard": 0, "modified": 1}


def _record(route, **figures):
    row = {k: float(v) for k, v in figures.items()}
    print(route, row)
    out = os.environ.get("SIMPLE_ACCURACY_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "simple_accuracy.json")
    try:
        rows = json.load(open(path))
    except (OSError, ValueError):
        rows = {}
    rows[route] = row
    json.dump(rows, open(path, "w"), indent=1, sort_keys=True)


class SimpleCall:
    """The tensors of one call; the workspace and every output start as 0xFF bytes."""

    def __init__(self, am, lm, labels, il, ll, topology, blank=0, stream=None):
        pkg.build()
        self.lib = _lib.load_simple()
        B, T, V = am.shape
        U = lm.shape[1]
        self.dims = (B, T, U, V)
        d = torch.device(DEV)
        self.am = torch.as_tensor(am, device=d).contiguous()
        self.lm = torch.as_tensor(lm, device=d).contiguous()
        self.labels = torch.as_tensor(labels, device=d).contiguous()
        self.il = torch.as_tensor(il, device=d)
        self.ll = torch.as_tensor(ll, device=d)
        self.ws = torch.full((_lib.simple_workspace_bytes(T, U, B),), 0xFF, dtype=torch.uint8, device=d)
        self.costs = torch.full((B,), float("nan"), device=d)
        self.bytes = {k: torch.full((n * 4,), 0xFF, dtype=torch.uint8, device=d)
                      for k, n in (("occ", B * T * U), ("g_am", B * T * V), ("g_lm", B * U * V))}
        self.out = {k: v.view(torch.float32) for k, v in self.bytes.items()}
        self.topo = TOPO_ID[topology]
        self.opts = _lib.make_options((stream or torch.cuda.current_stream()).cuda_stream, blank, T, U)

    def enqueue(self, l=0.0, a=0.0, scale=None, costs=True, grads=True, occ=True):
        B, T, U, V = self.dims
        return self.lib.compute_rnnt_loss_simple(
            self.am.data_ptr(), self.lm.data_ptr(), self.out["g_am"].data_ptr() if grads else None,
            self.out["g_lm"].data_ptr() if grads else None, self.out["occ"].data_ptr() if occ else None, self.labels.data_ptr(),
            self.ll.data_ptr(), self.il.data_ptr(), scale.data_ptr() if scale is not None else None, V, B, self.topo, l, a,
            self.costs.data_ptr() if costs else None, self.ws.data_ptr(), self.opts)

    def poison(self, costs=True, grads=True, occ=True):
        if grads:
            self.bytes["g_am"].fill_(0xFF)
            self.bytes["g_lm"].fill_(0xFF)
        if occ:
            self.bytes["occ"].fill_(0xFF)
        if costs:
            self.ws.fill_(0xFF)
            self.costs.fill_(float("nan"))

    def run(self, l=0.0, a=0.0, scale=None, costs=True, grads=True, occ=True):
        """Poisons what the call is to write (the workspace too when the call runs the forward), runs it, returns the results."""
        self.poison(costs, grads, occ)
        scale_t = None if scale is None else torch.tensor(np.asarray(scale), dtype=torch.float32, device=DEV)
        assert self.enqueue(l, a, scale_t, costs, grads, occ) == 0
        return self.result()

    def result(self):
        B, T, U, V = self.dims
        torch.cuda.synchronize()
        return dict(costs=self.costs.cpu().numpy().astype(np.float64), occ=self.out["occ"].cpu().numpy().reshape(B, T, U),
                    g_am=self.out["g_am"].cpu().numpy().reshape(B, T, V), g_lm=self.out["g_lm"].cpu().numpy().reshape(B, U, V))


def _same(x, y):
    return all(np.array_equal(x[k], y[k], equal_nan=True) for k in ("costs", "occ", "g_am", "g_lm"))


def _check(route, got, ref, il, ll, scale=None, grads=True):
    """Everything against the restatement `ref` with the fixed bars; exact zeros on padding and without a path."""
    B = len(ref["costs"])
    cs = np.ones(B) if scale is None else np.abs(np.broadcast_to(np.asarray(scale, np.float64), (B,)))
    c, c_ref = got["costs"], ref["costs"]
    fin = np.isfinite(c_ref)
    assert np.array_equal(c[~fin], c_ref[~fin])  # no path: +inf exactly
    dc = np.abs(c[fin] - c_ref[fin]) / np.maximum(1.0, np.abs(c_ref[fin]))
    keys = ("occ", "g_am", "g_lm") if grads else ("occ",)
    for k in keys:
        assert np.isfinite(got[k]).all(), k
    do = np.abs(got["occ"] - ref["occ"]).max()
    dg = 0.0
    if grads:
        for b in range(B):
            for k in ("g_am", "g_lm"):
                bar = max(cs[b], 1e-30) * max(1.0, np.abs(ref[k][b]).max() / max(cs[b], 1e-30))
                dg = max(dg, np.abs(got[k][b] - ref[k][b]).max() / bar)
    zeros_ok = True
    for b in range(B):
        Tb, Lb = int(il[b]), int(ll[b])
        zeros_ok &= not got["occ"][b, Tb:].any() and not got["occ"][b, :, Lb + 1:].any()
        if grads:
            zeros_ok &= not got["g_am"][b, Tb:].any() and not got["g_lm"][b, Lb + 1:].any()
        if not fin[b]:
            zeros_ok &= not any(got[k][b].any() for k in keys)
    _record(route, cost_rel=dc.max() if dc.size else 0.0, occ_abs=do, grad_over_bar=dg)
    assert dc.size == 0 or dc.max() <= CTOL
    assert do <= OTOL
    assert dg <= GTOL  # (dg is already divided by |cost_scale| max(1, max |reference|))
    assert zeros_ok
    return dc, do, dg


def _run_case(route, case, topology, blank=0, l=0.0, a=0.0, scale=None):
    am, lm, labels, il, ll = case
    got = SimpleCall(am, lm, labels, il, ll, topology, blank=blank).run(l=l, a=a, scale=scale)
    ref = sc.loss_and_grad(am, lm, labels, il, ll, blank, l, a, topology, cost_scale=scale)
    _check(f"{route}_{topology}", got, ref, il, ll, scale)
    return got, ref


# ---- 1. vocabulary edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
@pytest.mark.parametrize("V", [2, 28, 29, 31, 65, 129, 1024])
def test_vocabularies(V, topology):
    """The cell pass stages 64 symbols at a time and holds 16 in registers: 65 and 129 are one past one and two staged chunks, 28, 29
    and 31 end inside a register piece; the gradient passes run 16, 32 or 64 lanes along V (2; 28 ... 31; the others)."""
    for blank in (0, V // 2, V - 1):
        case = sc.case(3, 12, 7, V, seed=V + blank, blank=blank)
        assert not (case[2] == blank).any()
        got, _ = _run_case(f"vocab_V{V}_blank{blank}", case, topology, blank=blank, l=0.25, a=0.25)
        assert np.isfinite(got["costs"][0])


# ---- 2. lattice edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
def test_no_labels(topology):
    am, lm, labels, il, ll = sc.case(3, 9, 1, 28, seed=200)  # U = 1: L = 0 everywhere
    got, _ = _run_case("no_labels", (am, lm, labels, il, ll), topology)
    assert np.isfinite(got["costs"]).all()


@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
def test_one_frame(topology):
    am, lm, labels, il, ll = sc.case(3, 1, 4, 28, seed=201, ragged=False)
    ll[:] = [0, 1, 3]  # one frame: the standard lattice takes any L, the modified one at most one label
    sc.poison(am, lm, il, ll)
    got, _ = _run_case("one_frame", (am, lm, labels, il, ll), topology)
    assert np.array_equal(np.isfinite(got["costs"]), [True, True, topology == "standard"])


def test_more_labels_than_frames():
    """Modified: +inf and exact zeros (checked by _check for every utterance without a path); the standard lattice has paths."""
    am, lm, labels, il, ll = sc.case(3, 6, 9, 28, seed=202, ragged=False)
    il[:] = [6, 3, 5]
    ll[:] = [8, 4, 5]
    sc.poison(am, lm, il, ll)
    got, _ = _run_case("L_gt_T", (am, lm, labels, il, ll), "modified", l=0.25)
    assert np.array_equal(got["costs"] == np.inf, [True, True, False])
    got, _ = _run_case("L_gt_T", (am, lm, labels, il, ll), "standard", l=0.25)
    assert np.isfinite(got["costs"]).all()


@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
@pytest.mark.parametrize("U", [64, 65, 130])
def test_lattice_widths(U, topology):
    """One, two and three columns per lane of the one-wavefront sweep; more than one 32 x 32 tile of the cell pass both ways."""
    case = sc.case(2, U + 3 if topology == "modified" else 37, U, 5, seed=210 + U)
    got, _ = _run_case(f"width_U{U}", case, topology)
    assert np.isfinite(got["costs"][0])


# columns per lane K of the one-wavefront sweep: 1, 2, 3, 4, 6, 8, 12, 16 for U <= 64 K; beyond 1024 columns 1024 threads
# (16 wavefronts, the neighbour through LDS) with 2, 3, 4, 6, 8 columns per thread: one U past each switch
SWEEP_SWITCHES = {"K4": 193, "K6": 257, "K8": 385, "K12": 513, "K16": 769, "wide_K2": 1025, "wide_K3": 2049, "wide_K4": 3073,
                  "wide_K6": 4097, "wide_K8": 6145}


@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
@pytest.mark.parametrize("name", list(SWEEP_SWITCHES))
def test_sweep_geometries(name, topology):
    """V = 3, utterance 0 at full length L = U - 1 wherever the reference is affordable.
    Standard lattice: 4 frames; every column of every geometry carries mass and the value crosses every lane and wavefront boundary.
    Modified lattice (a path reaches column u at frame u at the earliest): T = U + 1 frames on the one-wavefront geometries, so
    every column carries mass there too; on the 1024-thread geometries 40 frames and L = 38 and 40 (the reference of a full
    lattice of 1025 ... 6145 squared cells is out of reach): the cell test with skew = 0, the stores of every column and the
    exchange run, the mass stays in the first wavefront."""
    U = SWEEP_SWITCHES[name]
    if topology == "standard":
        am, lm, labels, il, ll = sc.case(2, 4, U, 3, seed=U)
    else:
        wide = U > 1024
        am, lm, labels, il, ll = sc.case(2, 40 if wide else U + 1, U, 3, seed=U, ragged=False)
        il[1] = 40
        ll[:] = [38, 40] if wide else [U - 1, 30]
        sc.poison(am, lm, il, ll)
    got, ref = _run_case(f"sweep_{name}_U{U}", (am, lm, labels, il, ll), topology)
    # (the label edge into the last column; with T = L + 2 the last column's own blank edges hold little)
    assert np.isfinite(got["costs"]).all() and ref["occ"][0, :, max(ll[0] - 1, 0):ll[0] + 1].max() > 1e-3


@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
def test_ragged_batch(topology):
    am, lm, labels, il, ll = sc.case(7, 40, 21, 28, seed=240)
    assert il[0] == 40 and ll[0] == 20 and len(set(il)) > 3
    got, _ = _run_case("ragged_B7", (am, lm, labels, il, ll), topology, l=0.25, a=0.25)
    assert np.isfinite(got["costs"]).all()


# ---- 3. split peaks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
def test_split_peaks(topology):
    """am peaks at symbol 3, lm at symbol 7, 200 above the rest: exp(am - max am) exp(lm - max lm) is e^-200 e^0 or e^0 e^-200 at
    the two peaks and e^-400 elsewhere -- a zero sum in float32.  The direct route sees 200 + N(0,1) at both peaks."""
    am, lm, labels, il, ll = sc.case(2, 12, 6, 28, seed=300)
    am[..., 3] += 200.0
    lm[..., 7] += 200.0
    for l, a in ((0.0, 0.0), (0.25, 0.25)):
        got, ref = _run_case(f"split_peaks_l{l}_a{a}", (am, lm, labels, il, ll), topology, l=l, a=a)
        assert np.isfinite(got["costs"]).all() and np.isfinite(ref["costs"]).all()
        assert np.abs(ref["g_am"]).max() > 1e-2


# ---- 4. scales ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
def test_scales(topology):
    am, lm, labels, il, ll = sc.case(3, 9, 5, 28, seed=400)
    B = 3
    k = SimpleCall(am, lm, labels, il, ll, topology)
    for l, a in sc.SCALES:
        c_first = None
        for sname, scale in (("null", None), ("mixed", np.array([-2.0, 0.5, 3.0])), ("mean", np.full(B, 1.0 / B))):
            got = k.run(l=l, a=a, scale=scale)
            c_first = got["costs"] if c_first is None else c_first
            assert np.array_equal(got["costs"], c_first)  # the costs do not depend on the scale, bit for bit
            ref = sc.loss_and_grad(am, lm, labels, il, ll, 0, l, a, topology, cost_scale=scale)
            _check(f"scale_{sname}_l{l}_a{a}_{topology}", got, ref, il, ll, scale)
        assert np.isfinite(c_first).all()
    assert np.abs(k.run(l=1.0)["costs"] - k.run(a=1.0)["costs"]).max() > 1e-2  # the scales did something


# ---- 5. long paths ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_case(kind):
    if kind == "trained":
        return sc.trained_like_case(2, 600, 151, 28, seed=21)
    return sc.case(2, 600, 151, 28, seed=20, sigma={"n01": 1.0, "n08": 8.0}[kind])


@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
@pytest.mark.parametrize("kind", ["n01", "n08", "trained"])
def test_long_paths(kind, topology):
    am, lm, labels, il, ll = _long_case(kind)
    got, ref = _run_case(f"long_B2_T600_U151_V28_{kind}", (am, lm, labels, il, ll), topology)
    assert np.isfinite(ref["costs"]).all()


# ---- 6. against the existing ops ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
def test_without_scales_it_is_the_existing_op_on_the_sum(topology):
    am, lm, labels, il, ll = sc.case(4, 40, 21, 28, seed=600)
    got, ref = _run_case("sum_B4_T40_U21_V28", (am, lm, labels, il, ll), topology)
    t = lambda x: torch.as_tensor(x, device=DEV)  # noqa: E731
    acts = (t(np.nan_to_num(am))[:, :, None, :] + t(np.nan_to_num(lm))[:, None, :, :]).contiguous()
    c2, g2 = pkg.rnnt_loss_and_grad(acts, t(labels), t(il), t(ll), topology=topology)
    torch.cuda.synchronize()
    c2, g2 = c2.cpu().numpy().astype(np.float64), g2.cpu().numpy().astype(np.float64)
    assert (np.abs(c2 - got["costs"]) <= 2 * CTOL * np.maximum(1.0, np.abs(ref["costs"]))).all()
    for b in range(4):  # (a sum of up to 40 of the op's gradients, each within its bar of 1e-4: the two bars added)
        assert np.abs(g2[b].sum(1) - got["g_am"][b]).max() <= GTOL * (21 + max(1.0, np.abs(ref["g_am"][b]).max()))
        assert np.abs(g2[b].sum(0) - got["g_lm"][b]).max() <= GTOL * (40 + max(1.0, np.abs(ref["g_lm"][b]).max()))


# ---- 7. calling conventions ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
def test_split_and_replayed_calls_are_the_combined_call(topology):
    am, lm, labels, il, ll = sc.case(3, 20, 9, 28, seed=700)
    scale_np = np.array([0.5, -1.0, 2.0])
    scale = torch.tensor(scale_np, dtype=torch.float32, device=DEV)
    first = SimpleCall(am, lm, labels, il, ll, topology)
    base = first.run(l=0.25, a=0.25, scale=scale_np)
    assert np.isfinite(base["costs"]).all()
    assert _same(first.run(l=0.25, a=0.25, scale=scale_np), base)       # a second identical call
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):  # everything below on a stream of its own
        k = SimpleCall(am, lm, labels, il, ll, topology, stream=side)
        f = k.run(l=0.25, a=0.25, grads=False)                           # forward alone (poisoned workspace)
        assert np.array_equal(f["costs"], base["costs"]) and np.array_equal(f["occ"], base["occ"])
        g = k.run(l=0.25, a=0.25, scale=scale_np, costs=False, occ=False)  # gradient pass alone, from the workspace that forward left
        assert _same(g, base)
        g = k.run(l=0.25, a=0.25, scale=scale_np, costs=False, occ=True)   # once more, and the occupancies again
        assert _same(g, base)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        k.opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, k.dims[1], k.dims[2])
        assert k.enqueue(0.25, 0.25, scale) == 0
    for _ in range(2):
        k.poison()
        graph.replay()
        assert _same(k.result(), base)


# ---- 8. out-of-range lengths --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
@pytest.mark.parametrize("what,value", [("T", 0), ("T", 13), ("L", -1), ("L", 9)])
def test_out_of_range_lengths(what, value, topology):
    """maxT = 12, maxU = 9: that utterance is NaN on its clamped lattice and zero beside it, its neighbours are not touched."""
    am, lm, labels, il, ll = sc.case(3, 12, 9, 28, seed=800, ragged=False)
    il_bad, ll_bad = il.copy(), ll.copy()
    (il_bad if what == "T" else ll_bad)[1] = value
    got = SimpleCall(am, lm, labels, il_bad, ll_bad, topology).run(l=0.25)
    Tc, Lc = int(np.clip(il_bad[1], 1, 12)), int(np.clip(ll_bad[1], 0, 8))
    assert np.isnan(got["costs"][1])
    assert np.isnan(got["occ"][1, :Tc, :Lc + 1]).all() and np.isnan(got["g_am"][1, :Tc]).all() and np.isnan(got["g_lm"][1, :Lc + 1]).all()
    assert not got["occ"][1, Tc:].any() and not got["occ"][1, :, Lc + 1:].any() and not got["g_am"][1, Tc:].any() and not got["g_lm"][1, Lc + 1:].any()
    ref = sc.loss_and_grad(am, lm, labels, il, ll, l=0.25, topology=topology)
    keep = [0, 2]
    _check(f"bad_{what}{value}_{topology}", {k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in ref.items()}, il[keep], ll[keep])


# ---- 9. autograd --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
def test_autograd(topology):
    pkg.build()
    am, lm, labels, il, ll = sc.case(3, 9, 5, 28, seed=900)
    t = lambda x: torch.as_tensor(x, device=DEV)  # noqa: E731
    kw = dict(lm_only_scale=0.25, am_only_scale=0.25, topology=topology)
    c1, o1, ga1, gl1 = pkg.rnnt_loss_simple_and_grad(t(am), t(lm), t(labels), t(il), t(ll), **kw)
    x, y = torch.tensor(am, device=DEV, requires_grad=True), torch.tensor(lm, device=DEV, requires_grad=True)
    costs, occ = pkg.rnnt_loss_simple(x, y, t(labels), t(il), t(ll), **kw)
    assert not occ.requires_grad
    costs.sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(costs.detach(), c1) and torch.equal(occ, o1) and torch.equal(x.grad, ga1) and torch.equal(y.grad, gl1)
    w = np.array([0.5, -1.5, 2.0])
    x, y = torch.tensor(am, device=DEV, requires_grad=True), torch.tensor(lm, device=DEV, requires_grad=True)
    costs, occ = pkg.rnnt_loss_simple(x, y, t(labels), t(il), t(ll), **kw)
    (torch.tensor(w, dtype=torch.float32, device=DEV) * costs).sum().backward()
    torch.cuda.synchronize()
    got = dict(costs=costs.detach().cpu().numpy().astype(np.float64), occ=occ.cpu().numpy(), g_am=x.grad.cpu().numpy(), g_lm=y.grad.cpu().numpy())
    _check(f"autograd_weighted_{topology}", got, sc.loss_and_grad(am, lm, labels, il, ll, 0, 0.25, 0.25, topology, cost_scale=w), il, ll, w)


# ---- 10. end to end -----------------------------------------------------------------------------------------------------
def _two_pass_inputs():
    B, T, U, J, V = 2, 30, 12, 16, 12
    enc, pred, _, _, W2, b2, labels, il, ll = fc.joint_case(B, T, U, J, J, V, seed=1001)  # (the seed: see test_two_pass_end_to_end)
    rng = np.random.default_rng(1002)
    Wa, Wl = rng.normal(size=(J, V)).astype(np.float32) * 0.1, rng.normal(size=(J, V)).astype(np.float32) * 0.1
    return enc, pred, W2, b2, Wa, Wl, labels, il, ll


@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
def test_two_pass_end_to_end(topology):
    """rnnt_loss_two_pass at B2 T30 U12 J16 V12 S4 on the device against the same pipeline on the CPU mirrors: the same bands, costs
    within the bar, and the gradients of all four leaves.  No window of the CPU's occupancies ties within 1e-3 of the best one
    (checked here), so float32 occupancies choose the same bands."""
    pkg.build()
    S = 4
    enc, pred, W2, b2, Wa, Wl, labels, il, ll = _two_pass_inputs()

    def forward(dev):
        t = lambda x: torch.as_tensor(x, device=dev)  # noqa: E731
        e, p = torch.tensor(enc, device=dev, requires_grad=True), torch.tensor(pred, device=dev, requires_grad=True)
        am, lm = e @ t(Wa), p @ t(Wl)
        W, bias = t(W2), t(b2)
        s, pr, sb = pkg.rnnt_loss_two_pass(am, lm, e, p, lambda a, q: torch.tanh(a + q) @ W + bias, t(labels), t(il), t(ll), S,
                                           lm_only_scale=0.25, topology=topology)
        (0.5 * s.sum().to(torch.float32) + pr.sum().to(torch.float32)).backward()
        return e, p, s, pr, sb, am.detach(), lm.detach()

    e64, p64, s64, pr64, sb64, am, lm = forward("cpu")
    occ = pkg.rnnt_loss_simple(am, lm, *[torch.as_tensor(x) for x in (labels, il, ll)], lm_only_scale=0.25, topology=topology)[1].numpy()
    for b in range(2):
        hi = max(0, int(ll[b]) + 1 - S)
        for tt in range(1, int(il[b]) - 1):
            win = np.sort([occ[b, tt, s0:s0 + S].sum() for s0 in range(hi + 1)])
            assert len(win) < 2 or win[-1] - win[-2] > 1e-3, (b, tt)
    e, p, s, pr, sb, _, _ = forward(DEV)
    torch.cuda.synchronize()
    assert torch.equal(sb.cpu(), sb64)
    ds = (s.detach().cpu().double() - s64.detach()).abs() / s64.detach().abs().clamp(min=1.0)
    dp = (pr.detach().cpu().double() - pr64.detach()).abs() / pr64.detach().abs().clamp(min=1.0)
    de = (e.grad.cpu().double() - e64.grad.double()).abs().max().item() / max(1.0, e64.grad.abs().max().item())
    dq = (p.grad.cpu().double() - p64.grad.double()).abs().max().item() / max(1.0, p64.grad.abs().max().item())
    _record(f"two_pass_{topology}", simple_cost_rel=ds.max(), pruned_cost_rel=dp.max(), d_enc=de, d_pred=dq)
    assert torch.isfinite(s64).all() and torch.isfinite(pr64).all()
    assert ds.max() <= CTOL and dp.max() <= CTOL and de <= GTOL and dq <= GTOL
    assert e64.grad.abs().max() > 1e-2 and p64.grad.abs().max() > 1e-2
