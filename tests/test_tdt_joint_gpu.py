"""GPU tests of the fused TDT joint (include/rnnt_tdt_joint.h compute_rnnt_joint_loss_tdt) against the float64 restatement of
tests/tdt_joint_cases.py.

Bars: rnnt_pruned_joint.h's, taken over because the arithmetic is the same (tests/test_pruned_joint_gpu.py) -- costs and every
gradient tensor within 1e-4 max(1, max |reference|), gradients times |cost_scale|.  With M the largest |entry| of a gradient's
reference at unit cost_scale: an utterance's rows of d_enc_proj / d_pred_proj are within 1e-4 |cost_scale_b| max(1, M), and dW2 /
db2 (sums over the batch) within 1e-4 max |cost_scale| max(1, M); a cost within 1e-4 max(1, |cost|).  Rows of d_enc_proj beyond
T_b and of d_pred_proj beyond L_b, and everything of an utterance without a path, are exact zeros.
Every call through the C ABI gets gradient buffers and a workspace filled with 0xFF bytes (NaN; a gradient-only call: the
workspace its forward left); the rows of enc_proj beyond T_b and of pred_proj beyond L_b are NaN; W2 and b2 sit, exactly to size,
in front of NaN: a column beyond V + D that was loaded and not masked would arrive in the results.
The shapes are the smallest at which each mechanism can go wrong: the head boundary against the 32-column logit tile, a second
tile of 32 lattice columns with one live column, the chunk of 32 frames of the dh kernel, J = 64 ... 640.
The measured maxima are printed and, with TDT_JOINT_ACCURACY_DIR set, collected in tdt_joint_accuracy.json in that directory
(kept in profiles/tdt_joint_notes.md)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib
from rnnt_speech_recognition_amd import tdt_joint as tj_mod
from tests import tdt_joint_cases as tj

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
KEYS = tj.GRAD_KEYS
D5 = [0, 1, 2, 3, 4]
FRAME_CHUNK = 32  # csrc/rnnt_tdt_joint.h kTJFrameChunk: frames per workgroup of the dh kernel


def _record(route, **figures):
    row = {k: float(v) for k, v in figures.items()}
    print(route, row)
    out = os.environ.get("TDT_JOINT_ACCURACY_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "tdt_joint_accuracy.json")
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

    def __init__(self, case, durations, blank=0, sigma=0.0):
        pkg.build()
        self.lib = _lib.load_tdtjoint()
        d = torch.device(DEV)
        enc, pred = case["enc"], case["pred"]
        self.B, self.T, self.J = enc.shape
        self.U, self.R = pred.shape[1], case["W2"].shape[1]
        self.D = len(durations)
        self.V = self.R - self.D
        self.dur = (ctypes.c_int * self.D)(*durations)
        self.sigma = float(sigma)
        self.enc = torch.as_tensor(enc, device=d).contiguous()
        self.pred = torch.as_tensor(pred, device=d).contiguous()
        self.W2, self.b2 = _exact(case["W2"], d), _exact(case["b2"], d)
        self.labels = torch.as_tensor(case["labels"], device=d).contiguous()
        self.il = torch.as_tensor(case["il"], device=d)
        self.ll = torch.as_tensor(case["ll"], device=d)
        assert self.labels.shape[1] == max(self.U - 1, 1)
        self.ws = torch.full((_lib.tdt_joint_workspace_bytes(self.T, self.U, self.B, self.D, self.J),), 0xFF, dtype=torch.uint8, device=d)
        self.costs = torch.full((self.B,), float("nan"), device=d)
        self.shapes = ((self.B, self.T, self.J), (self.B, self.U, self.J), (self.J, self.R), (self.R,))
        self.gbytes = [torch.full((int(np.prod(s)) * 4,), 0xFF, dtype=torch.uint8, device=d) for s in self.shapes]
        self.opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, blank, self.T, self.U)

    def enqueue(self, scale=None, costs=True, grads=True):
        g = [b.data_ptr() if grads else None for b in self.gbytes]
        return self.lib.compute_rnnt_joint_loss_tdt(
            self.enc.data_ptr(), self.pred.data_ptr(), self.W2.data_ptr(), self.b2.data_ptr(), self.labels.data_ptr(),
            self.ll.data_ptr(), self.il.data_ptr(), scale.data_ptr() if scale is not None else None, self.J, self.V, self.dur, self.D,
            self.sigma, self.B, self.costs.data_ptr() if costs else None, g[0], g[1], g[2], g[3], self.ws.data_ptr(), self.opts)

    def run(self, scale=None, costs=True, grads=True):
        """Poisons what the call is to write (the workspace too when the call runs the forward), runs it, returns the results."""
        if grads:
            for b in self.gbytes:
                b.fill_(0xFF)
        if costs:
            self.ws.fill_(0xFF)
            self.costs.fill_(float("nan"))
        scale_t = None if scale is None else torch.tensor(np.asarray(scale), dtype=torch.float32, device=DEV)
        assert self.enqueue(scale_t, costs, grads) == 0
        return self.result()

    def result(self):
        torch.cuda.synchronize()
        out = dict(costs=self.costs.cpu().numpy().astype(np.float64))
        for key, b, s in zip(KEYS, self.gbytes, self.shapes):
            out[key] = b.view(torch.float32).cpu().numpy().reshape(s)
        return out


def _ref(case, durations, blank=0, sigma=0.0, scale=None):
    return tj.loss_and_grads(case["enc"], case["pred"], case["W2"], case["b2"], case["labels"], case["il"], case["ll"], durations,
                             blank, sigma, scale)


def _check(route, got, ref, case, scale=None, keep=None):
    """Costs and the four gradients against the restatement with the fixed bars; exact zeros where the contract has them.
    `keep`: the utterances to look at (the others are out of range: NaN, checked by the caller)."""
    B = len(ref["costs"])
    keep = np.arange(B) if keep is None else np.asarray(keep)
    cs = np.ones(B) if scale is None else np.abs(np.broadcast_to(np.asarray(scale, np.float64), (B,)))
    c, c_ref = got["costs"][keep], ref["costs"][keep]
    fin = np.isfinite(c_ref)
    assert np.array_equal(c[~fin], c_ref[~fin])  # no path: +inf exactly
    dc = np.abs(c[fin] - c_ref[fin]) / np.maximum(1.0, np.abs(c_ref[fin]))
    figures = dict(cost_rel=dc.max() if dc.size else 0.0)
    worst = figures["cost_rel"] / TOL
    for key in ("d_enc", "d_pred"):
        assert np.isfinite(got[key][keep]).all(), key
        units = [np.abs(ref[key][b]).max() / cs[b] for b in keep if cs[b] > 0]
        unit = max([1.0] + units)  # max |reference| at unit scale
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
    T, U = got["d_enc"].shape[1], got["d_pred"].shape[1]
    for b in keep:
        Tb, Lb = min(max(int(case["il"][b]), 1), T), min(max(int(case["ll"][b]), 0), U - 1)
        assert not got["d_enc"][b, Tb:].any() and not got["d_pred"][b, Lb + 1:].any(), b
        if not np.isfinite(ref["costs"][b]):
            assert not got["d_enc"][b].any() and not got["d_pred"][b].any(), b
    return figures


def _run_case(route, case, durations=D5, blank=0, sigma=0.0, scale=None):
    got = JointCall(case, durations, blank=blank, sigma=sigma).run(scale=scale)
    ref = _ref(case, durations, blank, sigma, scale)
    _check(route, got, ref, case, scale)
    return got, ref


# ---- 1. the head boundary against the 32-column logit tile --------------------------------------------------------------
@pytest.mark.parametrize("V,D", [(30, 5), (32, 4), (28, 8), (2, 1), (61, 3)])
def test_head_boundary(V, D):
    """(30, 5): the boundary inside a tile; (32, 4): on the tile edge; (28, 8): the duration head straddles two tiles; (2, 1): the
    smallest; (61, 3): the boundary in the second tile, which the heads share."""
    dur = [1] if D == 1 else list(range(D))
    for blank in (0, V - 1):
        case = tj.joint_case([(7, 4), (5, 2), (6, 0)], 64, V, D, seed=10 * V + D + blank, blank=blank)
        assert not (case["labels"] == blank).any()
        got, _ = _run_case(f"head_V{V}_D{D}_blank{blank}", case, dur, blank=blank)
        assert np.isfinite(got["costs"]).all()


def test_widest_alphabet():
    """V + D = 8192, the limit, on a 2 x 2 lattice."""
    case = tj.joint_case([(2, 1)], 64, 8187, 5, seed=8192)
    got, _ = _run_case("head_V8187_D5", case, D5)
    assert np.isfinite(got["costs"]).all()


# ---- 2. lattice columns -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [0, 31, 32])
def test_column_tiles(L):
    """U = 1 (no labels), U = 32 (one full tile of columns) and U = 33 (a second tile with one live column); L_b ragged across
    the batch, one utterance with L_b < maxU - 1 by a whole tile when there are two."""
    lengths = [(4, 0), (3, 0)] if L == 0 else [(5, L), (4, L // 2), (5, 1)]
    _run_case(f"columns_U{L + 1}", tj.joint_case(lengths, 64, 28, 5, seed=100 + L), [1, 2] if L == 0 else D5)


# ---- 3. frames ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, FRAME_CHUNK - 1, FRAME_CHUNK, FRAME_CHUNK + 1])
def test_frame_chunks(T):
    """T = 1, and one less than, equal to and one more than the dh kernel's chunk of frames; T_b ragged."""
    lengths = [(1, 0), (1, 0)] if T == 1 else [(T, 3), (T - 2, 2), (T // 2, 3)]
    _run_case(f"frames_T{T}", tj.joint_case(lengths, 64, 28, 5, seed=200 + T), [1] if T == 1 else D5)


# ---- 4. joint widths ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [64, 128, 640])
def test_joint_widths(J):
    got, _ = _run_case(f"width_J{J}", tj.joint_case([(6, 3), (5, 1)], J, 28, 5, seed=300 + J), D5)
    assert np.isfinite(got["costs"]).all()


# ---- 5. duration sets, paths, sigma, cost_scale -------------------------------------------------------------------------
@pytest.mark.parametrize("dur", [[0, 1, 2, 3, 4], [1], [1, 2], [0, 2], [1, 2, 3, 4, 5, 6, 7, 8]])
def test_duration_sets_with_and_without_a_path(dur):
    """One batch mixes utterances with and without a path: [0, 2] with an odd T and [1, 2] with L >= T have none; the others'
    results are untouched by them.  sigma > 0 and a cost_scale with a zero and a negative entry ride along."""
    lengths = [(8, 3), (7, 3), (3, 3), (6, 0)]
    case = tj.joint_case(lengths, 64, 28, len(dur), seed=400 + 10 * len(dur) + dur[-1])
    scale = [1.5, -2.0, 0.75, 0.0]
    got, ref = _run_case(f"durations_{'_'.join(map(str, dur))}", case, dur, sigma=0.05, scale=scale)
    if dur[0] == 1:  # every label consumes a frame and must land before T
        want = np.array([l < t for t, l in lengths])
    elif dur == [0, 2]:  # frames advance two at a time
        want = np.array([t % 2 == 0 for t, _ in lengths])
    else:
        want = np.ones(len(lengths), bool)
    assert np.array_equal(np.isfinite(ref["costs"]), want) and np.array_equal(np.isfinite(got["costs"]), want)
    assert (got["costs"][~want] == np.inf).all()


def test_cost_scale_and_call_modes_agree():
    """Forward-only, gradient-only twice with different cost_scale, and the combined call: the same bits where they compute the
    same thing, and each within the bars."""
    case = tj.joint_case([(9, 5), (7, 2), (8, 4)], 128, 30, 5, seed=500)
    s1, s2 = [2.0, -0.5, 0.0], [0.25, 3.0, -1.0]
    call = JointCall(case, D5, sigma=0.02)
    combined = call.run(scale=s1)
    fwd = call.run(grads=False)
    assert np.array_equal(fwd["costs"], combined["costs"])
    g1 = call.run(scale=s1, costs=False)
    g2 = call.run(scale=s2, costs=False)
    g1b = call.run(scale=s1, costs=False)
    for key in KEYS:
        assert np.array_equal(g1[key], combined[key]) and np.array_equal(g1[key], g1b[key]), key
    _check("modes_scale1", g1, _ref(case, D5, 0, 0.02, s1), case, s1)
    _check("modes_scale2", g2, _ref(case, D5, 0, 0.02, s2), case, s2)
    again = JointCall(case, D5, sigma=0.02).run(scale=s1)  # two identical calls: the same bits
    assert np.array_equal(again["costs"], combined["costs"])
    for key in KEYS:
        assert np.array_equal(again[key], combined[key]), key


def test_an_utterance_alone_equals_the_utterance_in_a_batch():
    case = tj.joint_case([(33, 33), (20, 7), (9, 40)], 64, 28, 5, seed=600)
    batch = JointCall(case, D5).run()
    for b in range(3):
        Tb, Lb = int(case["il"][b]), int(case["ll"][b])
        one = dict(enc=case["enc"][b:b + 1, :Tb].copy(), pred=case["pred"][b:b + 1, : Lb + 1].copy(), W2=case["W2"], b2=case["b2"],
                   labels=case["labels"][b:b + 1, : max(Lb, 1)].copy(), il=case["il"][b:b + 1], ll=case["ll"][b:b + 1])
        alone = JointCall(one, D5).run()
        assert np.array_equal(alone["costs"][0], batch["costs"][b])
        assert np.array_equal(alone["d_enc"][0], batch["d_enc"][b, :Tb]) and np.array_equal(alone["d_pred"][0], batch["d_pred"][b, : Lb + 1])
    _check("alone_batch", batch, _ref(case, D5), case)


@pytest.mark.parametrize("what,value", [("T", 0), ("T", 13), ("L", -1), ("L", 9)])
def test_out_of_range_lengths(what, value):
    """NaN for that utterance, as the header says; the others' costs, d_enc_proj and d_pred_proj are intact."""
    case = tj.joint_case([(9, 4), (8, 5), (7, 3)], 64, 28, 5, seed=700, poison=False)
    good = JointCall(case, D5).run()
    (case["il"] if what == "T" else case["ll"])[1] = value
    got = JointCall(case, D5).run()
    assert np.isnan(got["costs"][1]) and np.isnan(got["dW2"]).all() and np.isnan(got["db2"]).all()
    Tb, Lb = min(max(int(case["il"][1]), 1), 9), min(max(int(case["ll"][1]), 0), 5)
    assert np.isnan(got["d_enc"][1, :Tb]).all() and np.isnan(got["d_pred"][1, : Lb + 1]).all()
    assert not got["d_enc"][1, Tb:].any() and not got["d_pred"][1, Lb + 1:].any()
    for b in (0, 2):
        assert np.array_equal(got["costs"][b], good["costs"][b])
        assert np.array_equal(got["d_enc"][b], good["d_enc"][b]) and np.array_equal(got["d_pred"][b], good["d_pred"][b])
    _check("out_of_range", got, _ref(case, D5), case, keep=[0, 2])


@pytest.mark.parametrize("log2", [-20, 10])
def test_w2_magnitudes(log2):
    case = tj.joint_case([(7, 4), (6, 2)], 64, 28, 5, seed=800 + log2, w_scale=2.0 ** log2)
    _run_case(f"w2_scale_2^{log2}", case, D5)


# ---- 6. the Python routes -----------------------------------------------------------------------------------------------
def _tensors(case, dev):
    t = lambda x: torch.as_tensor(np.nan_to_num(x) if x.dtype == np.float32 else x, device=dev)  # noqa: E731
    return [t(case[k]) for k in ("enc", "pred", "W2", "b2", "labels", "il", "ll")]


def test_autograd_route_equals_the_combined_call():
    case = tj.joint_case([(9, 5), (7, 2)], 64, 30, 5, seed=900)
    enc, pred, W2, b2, labels, il, ll = _tensors(case, DEV)
    costs, *grads = tj_mod.rnnt_joint_loss_tdt_and_grad(enc, pred, W2, b2, labels, il, ll, D5, sigma=0.01)
    leaves = [x.clone().requires_grad_(True) for x in (enc, pred, W2, b2)]
    c2 = tj_mod.rnnt_joint_loss_tdt(*leaves, labels, il, ll, D5, sigma=0.01)
    c2.sum().backward()
    assert torch.equal(c2.detach(), costs)
    for leaf, g in zip(leaves, grads):
        assert torch.equal(leaf.grad, g)
    ref = _ref({**case, "enc": np.nan_to_num(case["enc"]), "pred": np.nan_to_num(case["pred"])}, D5, 0, 0.01)
    got = dict(costs=costs.cpu().numpy().astype(np.float64), **{k: g.cpu().numpy() for k, g in zip(KEYS, grads)})
    _check("python_route", got, ref, case)


def test_module_on_the_device_against_its_cpu_mirror():
    """TDTJointLoss with a J that needs padding (40 -> 64): all six gradients against the float64 mirror on the CPU."""
    from types import SimpleNamespace

    rng = np.random.default_rng(950)
    B, T, U, H, J, V = 2, 6, 4, 24, 40, 12
    mk = lambda *s, k=1.0: (k * rng.normal(size=s)).astype(np.float32)  # noqa: E731
    params = dict(W1=mk(H, J, k=0.3), b1=mk(J, k=0.1), W2=mk(J, V + 5, k=0.3), b2=mk(V + 5, k=0.1), enc=mk(B, T, H), pred=mk(B, U, H))
    labels = torch.as_tensor(rng.integers(1, V, size=(B, U - 1)).astype(np.int32))
    il, ll = torch.tensor([6, 5], dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32)
    out = {}
    for dev in ("cpu", DEV):
        t = {k: torch.as_tensor(v, device=dev).requires_grad_(True) for k, v in params.items()}
        joint = SimpleNamespace(W1=t["W1"], b1=t["b1"], W2=t["W2"], b2=t["b2"])
        costs = tj_mod.TDTJointLoss(D5, sigma=0.01)(joint, t["enc"], t["pred"], labels.to(dev), il.to(dev), ll.to(dev))
        (costs.double() * torch.tensor([1.0, -0.5], dtype=torch.float64, device=dev)).sum().backward()
        out[dev] = (costs.detach().cpu().double().numpy(), {k: v.grad.cpu().double().numpy() for k, v in t.items()})
    (c_cpu, g_cpu), (c_dev, g_dev) = out["cpu"], out[DEV]
    assert np.abs(c_dev - c_cpu).max() <= TOL * max(1.0, np.abs(c_cpu).max())
    for k in params:
        r = np.abs(g_dev[k] - g_cpu[k]).max() / max(1.0, np.abs(g_cpu[k]).max())
        _record(f"module_{k}", rel=r)
        assert r <= TOL, (k, r)
