"""GPU tests of FastEmit regularisation (include/rnnt.h compute_rnnt_loss_fastemit, compute_rnnt_joint_loss_bwd_fastemit,
compute_rnnt_joint_net_loss_bwd_fastemit) on every gradient route, at lambda = 0.5 (far above every bar), against the float64
restatement of tests/fastemit_cases.py.

Bars (the project's own fixed ones): the op -- costs within 1e-4 max(1, |cost|), gradients within 1e-4 absolute (include/rnnt.h);
the f32-grade joint -- 1e-4 max(1, max|ref|); the f16 joint -- costs 1e-4 relative and gradients 1e-3 max(1, max|ref|) against the
UNROUNDED float64 joint, the bar tests/test_joint_f16_gpu.py applies to its small shapes, with that file's weight recipe.
The measured maxima are printed and, with FASTEMIT_ACCURACY_DIR set, collected in fastemit_accuracy.json in that directory (kept as
profiles/fastemit_accuracy.json)."""
import json
import os

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib
from tests import fastemit_cases as fc
from tests.test_lin_gpu import Call

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAM = 0.5
INVALID = 2  # RNNT_STATUS_INVALID_VALUE


def _record(route, **figures):
    row = {k: float(v) for k, v in figures.items()}
    print(route, row)
    out = os.environ.get("FASTEMIT_ACCURACY_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "fastemit_accuracy.json")
    try:
        rows = json.load(open(path))
    except (OSError, ValueError):
        rows = {}
    rows[route] = row
    json.dump(rows, open(path, "w"), indent=1, sort_keys=True)


# ---- the op ---------------------------------------------------------------------------------------------------------------
def _fe(k, lam, scale=None, flags=0, costs=True, grads=True):
    """compute_rnnt_loss_fastemit on the buffers of a tests/test_lin_gpu.py Call; returns the status."""
    B, T, U, V = k.shape
    return k.lib.compute_rnnt_loss_fastemit(k.acts.data_ptr(), k.grads.data_ptr() if grads else None, k.labels.data_ptr(),
                                            k.ll.data_ptr(), k.il.data_ptr(), scale.data_ptr() if scale is not None else None, V, B,
                                            k.costs.data_ptr() if costs else None, k.ws.data_ptr(), k.opts, flags, lam)


def _flags(k, scale=None, flags=0):
    B, T, U, V = k.shape
    st = k.lib.compute_rnnt_loss_flags(k.acts.data_ptr(), k.grads.data_ptr(), k.labels.data_ptr(), k.ll.data_ptr(), k.il.data_ptr(),
                                       scale.data_ptr() if scale is not None else None, V, B, k.costs.data_ptr(), k.ws.data_ptr(),
                                       k.opts, flags)
    assert st == 0
    return k.result()


OP_ROUTES = {
    # route: (case builder, RNNT_VISIT_ALL, gradient buffer offset in floats)
    "linear_B3_T9_U5_V28": (lambda: fc.op_case(3, 9, 5, 28, seed=1), 0, 0),
    "hand_back_B2_T12_U6_V8": (fc.hand_back_case, 0, 0),
    "log_unaligned_B2_T7_U4_V31": (lambda: fc.op_case(2, 7, 4, 31, seed=2), 0, 1),
    "cell_wave_floor_B2_T7_U4_V96": (lambda: fc.op_case(2, 7, 4, 96, seed=3), 0, 0),
    "cell_wave_visit_all_B2_T7_U4_V96": (lambda: fc.op_case(2, 7, 4, 96, seed=3), 1, 0),
    "cell_wave_floor_trained_B2_T7_U4_V96": (lambda: fc.trained_like_case(2, 7, 4, 96, seed=4), 0, 0),
    "cell_wave_visit_all_trained_B2_T7_U4_V96": (lambda: fc.trained_like_case(2, 7, 4, 96, seed=4), 1, 0),
    "wide_sweep_B1_T3_U1030_V4": (lambda: fc.op_case(1, 3, 1030, 4, seed=5), 0, 0),
}


@pytest.mark.parametrize("route", sorted(OP_ROUTES))
def test_op_route(route):
    pkg.build()
    build, visit_all, off = OP_ROUTES[route]
    acts, labels, il, ll = build()
    B = acts.shape[0]
    flags = _lib.RNNT_VISIT_ALL if visit_all else 0
    scale_np = np.linspace(0.5, 2.0, B) if B > 1 else np.array([0.75])
    scale = torch.tensor(scale_np, dtype=torch.float32, device=DEV)
    k = Call(acts, labels, il, ll, grad_offset_floats=off)
    c0, g0 = _flags(k, scale, flags)                      # today's entry point
    assert _fe(k, 0.0, scale, flags) == 0                 # lambda = 0 through the new one: the same kernels, bit for bit
    cz, gz = k.result()
    assert np.array_equal(cz, c0) and np.array_equal(gz, g0)
    res = {}
    for lam in (1.0, LAM):
        k.gbuf.fill_(float("nan"))
        assert _fe(k, lam, scale, flags) == 0
        res[lam] = k.result()
        assert np.array_equal(res[lam][0], c0)            # the costs do not depend on lambda
    if route.startswith("hand_back"):
        f = k.flags()
        assert f[0, :2].any() and f[0, 3] == 2 and not f[1].any(), f
    c, g = res[LAM]
    c_ref, g_ref = fc.loss_and_grad(acts, labels, il, ll, LAM, scale_np)
    dc = np.abs(c - c_ref) / np.maximum(1.0, np.abs(c_ref))
    dg = np.abs(g - g_ref).max()
    d0 = np.abs(g0 - fc.loss_and_grad(acts, labels, il, ll, 0.0, scale_np)[1]).max()
    aff = np.abs(g - 0.5 * (g0.astype(np.float64) + res[1.0][1])).max()
    zs = np.abs(g.astype(np.float64).sum(-1)).max()
    _record("op/" + route, cost_rel=dc.max(), grad_abs=dg, grad_abs_lambda0=d0, affinity_abs=aff, zero_sum_abs=zs,
            effect_abs=np.abs(g - g0).max())
    assert dc.max() <= 1e-4 and dg <= 1e-4 and aff <= 1e-4 and zs <= 1e-4
    assert np.abs(g - g0).max() > 1e-2  # lambda did something
    for b in range(B):  # padded cells: exact zeros
        assert not g[b, il[b]:].any() and not g[b, :, ll[b] + 1:].any()
    # the gradient pass alone (costs == NULL) over the same forward, with another lambda: its own reference
    k.gbuf.fill_(float("nan"))
    assert _fe(k, 0.25, scale, flags, costs=False) == 0
    g25 = k.result()[1]
    assert np.abs(g25 - fc.loss_and_grad(acts, labels, il, ll, 0.25, scale_np)[1]).max() <= 1e-4


@pytest.mark.parametrize("V", [28, 96])
def test_rows_without_labels_do_not_depend_on_lambda(V):
    pkg.build()
    # U = 1: no labels at all
    acts, labels, il, ll = fc.op_case(2, 6, 1, V, seed=6)
    k = Call(acts, labels, il, ll)
    c0, g0 = _flags(k)
    assert _fe(k, LAM) == 0
    c, g = k.result()
    assert np.array_equal(c, c0) and np.array_equal(g, g0)
    # label_length = 0 in one row of a batch with labels
    acts, labels, il, ll = fc.op_case(3, 6, 4, V, seed=7)
    ll[1] = 0
    k = Call(acts, labels, il, ll)
    c0, g0 = _flags(k)
    assert _fe(k, LAM) == 0
    c, g = k.result()
    assert np.array_equal(c, c0) and np.array_equal(g[1], g0[1]) and not np.array_equal(g[0], g0[0])


@pytest.mark.parametrize("lam", [-0.1, 1.5, float("nan"), float("inf")])
def test_invalid_lambda_writes_nothing(lam):
    pkg.build()
    acts, labels, il, ll = fc.op_case(2, 5, 3, 28, seed=8)
    k = Call(acts, labels, il, ll)
    k.gbuf.fill_(-7.0)
    k.costs.fill_(-7.0)
    assert _fe(k, lam) == INVALID
    c, g = k.result()
    assert (c == -7.0).all() and (g == -7.0).all()
    j = JointCall(fc.proj_case(2, 5, 3, 64, 28, seed=8), 0)
    j.fwd()
    for out in j.outs:
        out.fill_(-7.0)
    assert j.bwd(lam) == INVALID
    torch.cuda.synchronize()
    assert all((o == -7.0).all().item() for o in j.outs)


def test_out_of_range_lengths_still_give_nan_for_that_utterance_only():
    pkg.build()
    acts, labels, il, ll = fc.op_case(3, 6, 4, 28, seed=9)
    good = fc.loss_and_grad(acts[[0, 2]], labels[[0, 2]], il[[0, 2]], ll[[0, 2]], LAM)
    il[1] = 99
    k = Call(acts, labels, il, ll)
    assert _fe(k, LAM) == 0
    c, g = k.result()
    # (the lengths are clamped into the tensor: NaN in every cell of the clamped lattice, zeros in its padded columns)
    assert np.isnan(c[1]) and np.isnan(g[1, :, : ll[1] + 1]).all() and not g[1, :, ll[1] + 1:].any()
    assert np.abs(c[[0, 2]] - good[0]).max() <= 1e-4 * np.abs(good[0]).max() and np.abs(g[[0, 2]] - good[1]).max() <= 1e-4


# ---- the fused joints through the C ABI -----------------------------------------------------------------------------------
class JointCall:
    """compute_rnnt_joint_loss_fwd / _bwd / _bwd_fastemit on one workspace (projections in, four gradients out)."""

    def __init__(self, case, joint_dtype, scale=None):
        self.lib = _lib.load()
        ep, pp, _, _, W2, b2, labels, il, ll = case
        d = torch.device(DEV)
        t = lambda x: torch.tensor(np.ascontiguousarray(x), device=d)
        self.ep, self.pp, self.W2, self.b2, self.labels, self.il, self.ll = (t(x) for x in (ep, pp, W2, b2, labels, il, ll))
        self.B, self.T, self.J = ep.shape
        self.U, self.V = pp.shape[1], W2.shape[1]
        self.dtype = joint_dtype
        self.scale = None if scale is None else torch.tensor(scale, dtype=torch.float32, device=d)
        self.ws = torch.empty(_lib.joint_workspace_bytes(self.T, self.U, self.B, self.J, self.V), dtype=torch.uint8, device=d)
        self.costs = torch.full((self.B,), float("nan"), device=d)
        self.outs = [torch.full_like(x, float("nan")) for x in (self.ep, self.pp, self.W2, self.b2)]
        self.opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, self.T, self.U)

    def _head(self):
        return [x.data_ptr() for x in (self.ep, self.pp, self.W2, self.b2, self.labels, self.ll, self.il)]

    def fwd(self):
        st = self.lib.compute_rnnt_joint_loss_fwd(*self._head(), self.J, self.V, self.B, self.costs.data_ptr(), self.dtype,
                                                  self.ws.data_ptr(), self.opts)
        assert st == 0
        torch.cuda.synchronize()
        return self.costs.cpu().numpy().astype(np.float64)

    def bwd(self, lam=None):
        args = self._head() + [self.scale.data_ptr() if self.scale is not None else None, self.J, self.V, self.B] + \
            [o.data_ptr() for o in self.outs] + [self.dtype, self.ws.data_ptr(), self.opts]
        if lam is None:
            return self.lib.compute_rnnt_joint_loss_bwd(*args)
        return self.lib.compute_rnnt_joint_loss_bwd_fastemit(*args, lam)

    def grads(self, lam=None):
        for o in self.outs:
            o.fill_(float("nan"))
        assert self.bwd(lam) == 0
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in self.outs]


PROJ_KEYS = ("d_a", "d_c", "dW2", "db2")


def _errs(got, ref, keys):
    return {k: float(np.abs(g - ref[k]).max() / max(1.0, np.abs(ref[k]).max())) for g, k in zip(got, keys)}


@pytest.mark.parametrize("J,V", [(64, 28), (128, 64), (704, 28)])
def test_f32_joint(J, V):
    pkg.build()
    case = fc.proj_case(2, 8, 5, J, V, seed=J + V)
    scale = np.array([0.5, 1.5])
    j = JointCall(case, 0, scale)
    c = j.fwd()
    plain = j.grads(None)
    zero = j.grads(0.0)  # lambda = 0 through the new entry point: bit-identical
    assert all(np.array_equal(a, b) for a, b in zip(plain, zero))
    one, half, quarter = j.grads(1.0), j.grads(LAM), j.grads(0.25)  # several calls over one forward, each its own reference
    assert np.array_equal(j.costs.cpu().numpy().astype(np.float64), c)
    ref = fc.joint_loss_and_grads(*case, LAM, cost_scale=scale)
    e = _errs(half, ref, PROJ_KEYS)
    e25 = _errs(quarter, fc.joint_loss_and_grads(*case, 0.25, cost_scale=scale), PROJ_KEYS)
    e0 = _errs(plain, fc.joint_loss_and_grads(*case, 0.0, cost_scale=scale), PROJ_KEYS)
    aff = {k: float(np.abs(h - 0.5 * (p.astype(np.float64) + o)).max() / max(1.0, np.abs(ref[k]).max()))
           for h, p, o, k in zip(half, plain, one, PROJ_KEYS)}
    cost_rel = float((np.abs(c - ref["costs"]) / np.maximum(1.0, np.abs(ref["costs"]))).max())
    _record(f"joint_f32/B2_T8_U5_J{J}_V{V}", cost_rel=cost_rel, **{"err_" + k: v for k, v in e.items()},
            **{"err_lambda0_" + k: v for k, v in e0.items()}, **{"affinity_" + k: v for k, v in aff.items()})
    assert cost_rel <= 1e-4
    assert max(e.values()) <= 1e-4 and max(e25.values()) <= 1e-4 and max(aff.values()) <= 1e-4, (e, e25, aff)
    assert np.abs(half[0] - plain[0]).max() > 1e-3


def test_f16_joint_first_and_second_backward():
    pkg.build()
    case = fc.proj_case(2, 8, 5, 128, 128, seed=11)
    case = case[:4] + (case[4] * 3.0,) + case[5:]  # tests/test_joint_f16_gpu.py's weight recipe: W2 x 3
    scale = np.array([0.5, 1.5])
    fig = {}
    results = {}
    for lam_first, lam_second in ((LAM, 0.25), (0.0, 0.0), (1.0, 1.0)):
        j = JointCall(case, 1, scale)
        c = j.fwd()
        first = j.grads(lam_first)    # the parked values
        second = j.grads(lam_second)  # consumed: the logits are recomputed
        results[lam_first] = (first, second)
        for tag, lam, got in (("parked", lam_first, first), ("recompute", lam_second, second)):
            ref = fc.joint_loss_and_grads(*case, lam, cost_scale=scale)
            e = _errs(got, ref, PROJ_KEYS)
            fig.update({f"{tag}_lambda{lam:g}_{k}": v for k, v in e.items()})
            assert max(e.values()) <= 1e-3, (tag, lam, e)
        np.testing.assert_allclose(c, ref["costs"], rtol=1e-4)
    # lambda = 0 through the new entry point against the existing one, both routes: bit-identical
    j = JointCall(case, 1, scale)
    j.fwd()
    p1, p2 = j.grads(None), j.grads(None)
    assert all(np.array_equal(a, b) for a, b in zip(results[0.0][0], p1)) and all(np.array_equal(a, b) for a, b in zip(results[0.0][1], p2))
    ref = fc.joint_loss_and_grads(*case, LAM, cost_scale=scale)
    aff = {k: float(np.abs(h - 0.5 * (z.astype(np.float64) + o)).max() / max(1.0, np.abs(ref[k]).max()))
           for h, z, o, k in zip(results[LAM][0], results[0.0][0], results[1.0][0], PROJ_KEYS)}
    fig.update({"affinity_parked_" + k: v for k, v in aff.items()})
    _record("joint_f16/B2_T8_U5_J128_V128", **fig)
    assert max(aff.values()) <= 1e-3, aff


# ---- the whole joint network, through the Python surface ---------------------------------------------------------------------
def _net(case, joint_dtype, lam, scale):
    t = lambda x: torch.tensor(x, device=DEV)
    params = [t(x).requires_grad_(True) for x in case[:6]]
    costs = pkg.rnnt_joint_loss(*params, t(case[6]), t(case[7]), t(case[8]), joint_dtype=joint_dtype, first_layer="engine",
                                fastemit_lambda=lam)
    (costs * t(scale.astype(np.float32))).sum().backward()
    torch.cuda.synchronize()
    return costs.detach().cpu().numpy(), [p.grad.cpu().numpy() for p in params]


@pytest.mark.parametrize("joint_dtype,J,V,bar", [("f32", 64, 28, 1e-4), ("f16", 128, 128, 1e-3)])
def test_whole_joint_network(joint_dtype, J, V, bar, monkeypatch):
    pkg.build()
    case = fc.joint_case(2, 8, 5, 32, J, V, seed=13, f16_recipe=joint_dtype == "f16")
    scale = np.array([0.5, 1.5])
    c0, g0 = _net(case, joint_dtype, 0.0, scale)
    c, g = _net(case, joint_dtype, LAM, scale)
    c1, g1 = _net(case, joint_dtype, 1.0, scale)
    assert np.array_equal(c, c0)
    ref = fc.joint_loss_and_grads(*case, LAM, cost_scale=scale)
    e = _errs(g, ref, fc.GRAD_KEYS)
    e0 = _errs(g0, fc.joint_loss_and_grads(*case, 0.0, cost_scale=scale), fc.GRAD_KEYS)
    aff = {k: float(np.abs(h - 0.5 * (z.astype(np.float64) + o)).max() / max(1.0, np.abs(ref[k]).max()))
           for h, z, o, k in zip(g, g0, g1, fc.GRAD_KEYS)}
    _record(f"joint_net_{joint_dtype}/B2_T8_U5_H32_J{J}_V{V}", **{"err_" + k: v for k, v in e.items()},
            **{"err_lambda0_" + k: v for k, v in e0.items()}, **{"affinity_" + k: v for k, v in aff.items()})
    np.testing.assert_allclose(c, ref["costs"], rtol=1e-4)
    assert max(e.values()) <= bar and max(aff.values()) <= bar, (e, aff)
    # lambda = 0 through the new entry point (in place of the existing one under the autograd function): bit-identical
    lib = _lib.load()
    monkeypatch.setattr(lib, "compute_rnnt_joint_net_loss_bwd", lambda *a: lib.compute_rnnt_joint_net_loss_bwd_fastemit(*a, 0.0))
    cz, gz = _net(case, joint_dtype, 0.0, scale)
    assert np.array_equal(cz, c0) and all(np.array_equal(a, b) for a, b in zip(gz, g0))


def test_transducer_trains_with_fastemit():
    """Transducer(hp, fastemit_lambda=0.5).loss(...).backward() on tests/test_model.py's smallest configuration: the joint's six
    gradients against the float64 joint restatement fed with the model's own encoder / prediction-network outputs."""
    pkg.build()
    torch.manual_seed(0)
    hp = pkg.HParams(vocab_size=28, mel_bins=8, downsample_factor=3, embedding_size=16, encoder_layers=2, encoder_size=48,
                     projection_size=32, time_reduction_index=0, time_reduction_factor=2, pred_net_layers=1, pred_net_size=48,
                     joint_net_size=64, learning_rate=1e-3)
    m = pkg.Transducer(hp, fastemit_lambda=LAM).to(DEV)
    mel, pred_inp, spec_len, lab_len, labels = pkg.synthetic_batch(hp, batch=3, frames=12, max_labels=4, device=DEV, seed=2)
    m.train()
    seen = {}

    def keep(name):
        def hook(_module, _inputs, out):
            out.retain_grad()
            seen[name] = out
        return hook

    m.encoder.register_forward_hook(keep("enc"))
    m.prediction.register_forward_hook(keep("pred"))
    t_len = pkg.reduced_lengths(spec_len, hp.time_reduction_factor)
    costs = m.loss(mel, pred_inp, spec_len, lab_len, labels)
    (costs.sum() / 3).backward()
    enc, pred = seen["enc"], seen["pred"]
    torch.cuda.synchronize()
    n = lambda x: x.detach().cpu().numpy()
    jt = m.joint
    ref = fc.joint_loss_and_grads(n(enc), n(pred), n(jt.W1), n(jt.b1), n(jt.W2), n(jt.b2), n(labels), n(t_len), n(lab_len), LAM,
                                  cost_scale=np.full(3, 1.0 / 3))
    got = [n(enc.grad), n(pred.grad), n(jt.W1.grad), n(jt.b1.grad), n(jt.W2.grad), n(jt.b2.grad)]
    e = _errs(got, ref, fc.GRAD_KEYS)
    _record("transducer/test_model_small_hp", **{"err_" + k: v for k, v in e.items()})
    np.testing.assert_allclose(n(costs), ref["costs"], rtol=1e-4)
    assert max(e.values()) <= 1e-4, e
    plain = fc.joint_loss_and_grads(n(enc), n(pred), n(jt.W1), n(jt.b1), n(jt.W2), n(jt.b2), n(labels), n(t_len), n(lab_len), 0.0,
                                    cost_scale=np.full(3, 1.0 / 3))
    assert np.abs(plain["dW2"] - ref["dW2"]).max() > 1e-3  # not the plain loss's gradients
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
