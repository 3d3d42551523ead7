"""CPU tests of the fused joint on the pruned band: they pin the float64 restatement of tests/pruned_joint_cases.py against the
existing pruned restatement, the existing torch mirror and finite differences, the torch mirror of pruned_joint.py against that
restatement, and check what needs no device: argument errors, the export table of libwarprnnt_prunedjoint.so, its domain checks,
and rnnt_loss_two_pass_fused against rnnt_loss_two_pass with the torch joint."""
import ctypes

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib, pruned_joint, pruning
from tests import pruned_cases as pc
from tests import pruned_joint_cases as pj

INVALID = 2


@pytest.fixture(scope="module")
def lib():
    pkg.build()
    return _lib.load_prunedjoint()


def _t(case, *names):
    return [torch.as_tensor(case[n]) for n in names]


def _mirror(case, lam=0.0, scale=None, blank=0, topology="standard"):
    enc, pred, W2, b2, sb, labels, il, ll = _t(case, "enc", "pred", "W2", "b2", "sb", "labels", "il", "ll")
    cs = None if scale is None else torch.as_tensor(np.asarray(scale, np.float64))
    out = pruned_joint._mirror(enc, pred, W2, b2, sb, labels, il, ll, case["S"], blank, lam, topology, cs)
    return dict(zip(("costs",) + pj.GRAD_KEYS, (o.numpy() for o in out)))


def _ref(case, lam=0.0, scale=None, blank=0, topology="standard"):
    return pj.loss_and_grads(case["enc"], case["pred"], case["W2"], case["b2"], case["sb"], case["labels"], case["il"], case["ll"],
                             case["S"], lam, scale, blank, topology)


def _costs_agree(got, ref, tol=1e-10):
    """+inf (a band that does not connect) exactly, the rest within tol; returns which are finite."""
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin])
    assert not fin.any() or np.abs(got[fin] - ref[fin]).max() <= tol
    return fin


# ---- the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
def test_restatement_is_the_pruned_restatement_on_float64_logits(topology):
    """Costs: the existing restatement and the existing mirror on the logits the composed route forms.  Gradients: the existing
    restatement's dlogits pushed through a float64 torch joint by autograd."""
    case = pj.joint_case(3, 9, 5, 3, 8, 6, seed=1, steps=[0, 1])
    ref = _ref(case, lam=0.25, topology=topology)
    assert np.isfinite(ref["costs"]).all()
    x = pj.composed_logits(case["enc"], case["pred"], case["W2"], case["b2"], case["sb"], case["il"], case["ll"], 3)
    c_old, g_old = pc.loss_and_grad(x, case["sb"], case["labels"], case["il"], case["ll"], 0.25, topology=topology)
    assert np.abs(ref["costs"] - c_old).max() <= 1e-12
    c_m, _ = pruning._mirror(torch.as_tensor(x), torch.as_tensor(case["sb"]), torch.as_tensor(case["labels"]),
                             torch.as_tensor(case["il"]), torch.as_tensor(case["ll"]), 0, 0.25, topology, 6)
    assert np.abs(ref["costs"] - c_m.numpy()).max() <= 1e-10
    # autograd through the clamped gather of prune_joint_inputs: absent slots carry zero dlogits, so the clamp does not matter
    e = torch.tensor(np.nan_to_num(case["enc"]), dtype=torch.float64, requires_grad=True)
    p = torch.tensor(np.nan_to_num(case["pred"]), dtype=torch.float64, requires_grad=True)
    W = torch.tensor(case["W2"], dtype=torch.float64, requires_grad=True)
    bias = torch.tensor(case["b2"], dtype=torch.float64, requires_grad=True)
    a, q = pkg.prune_joint_inputs(e, p, torch.as_tensor(case["sb"]), 3)
    (torch.tanh(a + q) @ W + bias).backward(torch.as_tensor(g_old))
    for key, t in zip(pj.GRAD_KEYS, (e, p, W, bias)):
        assert np.abs(ref[key] - t.grad.numpy()).max() <= 1e-12, key


@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
def test_restatement_gradients_are_finite_differences(topology):
    case = pj.joint_case(2, 5, 3, 2, 4, 5, seed=2, ragged=False, steps=[0, 1])
    scale = np.array([0.5, -1.5])
    ref = _ref(case, scale=scale, topology=topology)  # (lambda = 0: FastEmit's gradient is not the gradient of the cost)
    rng = np.random.default_rng(3)
    eps = 1e-6
    for key, name in zip(pj.GRAD_KEYS, ("enc", "pred", "W2", "b2")):
        base = case[name].astype(np.float64)
        finite = np.argwhere(np.isfinite(base))
        for idx in finite[rng.choice(len(finite), size=min(6, len(finite)), replace=False)]:
            idx = tuple(idx)
            vals = []
            for d in (eps, -eps):
                moved = base.copy()
                moved[idx] += d
                vals.append(float((scale * _ref({**case, name: moved}, topology=topology)["costs"]).sum()))
            assert abs((vals[0] - vals[1]) / (2 * eps) - ref[key][idx]) <= 1e-6, (key, idx)


# ---- the mirror ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
def test_mirror_equals_restatement_on_ragged_batches(topology):
    for S, blank in ((1, 0), (3, 2), (5, 6)):
        case = pj.joint_case(4, 11, 6, S, 64, 7, seed=10 + S, blank=blank, steps=[0, 1])
        scale = np.array([1.0, -0.5, 2.0, 0.25])
        got, ref = _mirror(case, 0.01, scale, blank, topology), _ref(case, 0.01, scale, blank, topology)
        _costs_agree(got["costs"], ref["costs"])
        for key in pj.GRAD_KEYS:
            assert np.abs(got[key] - ref[key]).max() <= 1e-10, key


@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
def test_mirror_equals_restatement_on_hostile_ranges(topology):
    """NaN sits in every row of enc beyond T_b and of pred beyond L_b: nothing of it may arrive anywhere."""
    case = pj.hostile_case()
    got, ref = _mirror(case, 0.01, topology=topology), _ref(case, 0.01, topology=topology)
    assert ref["costs"][0] == np.inf and ref["costs"][3] == np.inf and ref["costs"][4] == np.inf
    assert (ref["costs"][8] == np.inf) == (topology == "modified")
    fin = _costs_agree(got["costs"], ref["costs"])
    rows_e, rows_p = pj.touched_rows(case["sb"], case["il"], case["ll"], 4, 10, 8)
    for key in pj.GRAD_KEYS:
        assert np.isfinite(got[key]).all() and np.abs(got[key] - ref[key]).max() <= 1e-10, key
    assert not got["d_enc"][~rows_e].any() and not got["d_pred"][~rows_p].any()
    assert not got["d_enc"][~fin].any() and not got["d_pred"][~fin].any()


@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
@pytest.mark.parametrize("what,value", [("T", 0), ("T", 13), ("L", -1), ("L", 9)])
def test_out_of_range_lengths(what, value, topology):
    case = pj.joint_case(3, 12, 8, 5, 64, 9, seed=20, ragged=False, line=True)
    good = _ref(case, topology=topology)
    assert np.isfinite(good["costs"]).all()
    (case["il"] if what == "T" else case["ll"])[1] = value
    got, ref = _mirror(case, topology=topology), _ref(case, topology=topology)
    assert np.isnan(got["costs"][1]) and np.isnan(ref["costs"][1])
    for b in (0, 2):
        assert abs(got["costs"][b] - good["costs"][b]) <= 1e-10
        assert np.abs(got["d_enc"][b] - good["d_enc"][b]).max() <= 1e-10 and np.abs(got["d_pred"][b] - good["d_pred"][b]).max() <= 1e-10
    rows_e, rows_p = pj.touched_rows(case["sb"], case["il"], case["ll"], 5, 12, 9)
    for g in (got, ref):
        assert np.isnan(g["d_enc"][1][rows_e[1]]).all() and not g["d_enc"][1][~rows_e[1]].any()
        assert np.isnan(g["d_pred"][1][rows_p[1]]).all() and not g["d_pred"][1][~rows_p[1]].any()
        assert np.isnan(g["dW2"]).all() and np.isnan(g["db2"]).all()


def test_public_functions_on_cpu_tensors():
    case = pj.joint_case(2, 8, 4, 3, 64, 6, seed=30, steps=[0, 1])
    enc, pred, W2, b2, sb, labels, il, ll = _t(case, "enc", "pred", "W2", "b2", "sb", "labels", "il", "ll")
    ref = _ref(case, 0.01)
    out = pkg.rnnt_joint_loss_pruned_and_grad(enc, pred, W2, b2, sb, labels, il, ll, fastemit_lambda=0.01, s_range=3)
    assert out[0].dtype == torch.float64 and np.abs(out[0].numpy() - ref["costs"]).max() <= 1e-10
    w = np.array([0.5, -2.0])
    ref_w = _ref(case, 0.01, w)
    leaves = [x.clone().requires_grad_(True) for x in (enc, pred, W2, b2)]  # (the NaN rows stay: nothing reads them)
    ranges = sb[:, :, None] + torch.arange(3, dtype=torch.int32)  # k2's [B, T, S] form: no s_range needed
    costs = pkg.rnnt_joint_loss_pruned(*leaves, ranges, labels, il, ll, fastemit_lambda=0.01)
    (torch.as_tensor(w) * costs).sum().backward()
    for key, leaf in zip(pj.GRAD_KEYS, leaves):
        assert leaf.grad.dtype == torch.float32 and np.abs(leaf.grad.numpy() - ref_w[key]).max() <= 1e-5, key


@pytest.mark.parametrize("topology", pj.TOPOLOGIES)
def test_two_pass_fused_is_two_pass_with_the_torch_joint(topology):
    B, T, U, J, V, S = 2, 12, 6, 64, 9, 3
    rng = np.random.default_rng(40)
    mk = lambda *shape: torch.tensor(rng.normal(size=shape), dtype=torch.float32)  # noqa: E731
    am, lm, enc, pred = mk(B, T, V), mk(B, U, V), mk(B, T, J), mk(B, U, J)
    W2, b2 = mk(J, V) * 0.2, mk(V) * 0.1
    labels = torch.tensor(rng.integers(1, V, size=(B, U - 1)), dtype=torch.int32)
    il, ll = torch.tensor([T, T - 3]), torch.tensor([U - 1, U - 3])

    def run(fused):
        leaves = [x.clone().requires_grad_(True) for x in (am, lm, enc, pred, W2, b2)]
        a, l, e, p, W, bias = leaves
        if fused:
            sc, pcost, sb = pkg.rnnt_loss_two_pass_fused(a, l, e, p, W, bias, labels, il, ll, S, fastemit_lambda=0.01, topology=topology)
        else:
            sc, pcost, sb = pkg.rnnt_loss_two_pass(a, l, e, p, lambda x, y: torch.tanh(x + y) @ W + bias, labels, il, ll, S,
                                                   fastemit_lambda=0.01, topology=topology)
        (0.5 * sc.sum() + pcost.sum()).backward()
        return sc.detach(), pcost.detach(), sb, [x.grad for x in leaves]

    s1, p1, sb1, g1 = run(True)
    s0, p0, sb0, g0 = run(False)
    assert torch.equal(sb1, sb0) and torch.equal(s1, s0) and torch.isfinite(p0).all()
    assert (p1 - p0).abs().max() <= 1e-4  # (the composed route's logits are float32)
    for x, y in zip(g1, g0):
        assert (x - y).abs().max() <= 1e-4
    assert g1[2].abs().max() > 1e-2 and g1[4].abs().max() > 1e-2


# ---- arguments ----------------------------------------------------------------------------------------------------------
def test_python_argument_errors():
    enc, pred, W2, b2 = torch.zeros(2, 4, 64), torch.zeros(2, 3, 64), torch.zeros(64, 5), torch.zeros(5)
    sb = torch.zeros(2, 4, dtype=torch.int32)
    rest = (torch.ones(2, 2, dtype=torch.int32), torch.tensor([4, 4]), torch.tensor([2, 2]))
    for fn in (pkg.rnnt_joint_loss_pruned, pkg.rnnt_joint_loss_pruned_and_grad):
        with pytest.raises(ValueError, match="enc_proj"):
            fn(enc[0], pred, W2, b2, sb, *rest, s_range=3)
        with pytest.raises(ValueError, match="pred_proj"):
            fn(enc, torch.zeros(2, 3, 128), W2, b2, sb, *rest, s_range=3)
        with pytest.raises(ValueError, match="W2"):
            fn(enc, pred, torch.zeros(32, 5), b2, sb, *rest, s_range=3)
        with pytest.raises(ValueError, match="W2"):
            fn(enc, pred, W2, torch.zeros(6), sb, *rest, s_range=3)
        with pytest.raises(ValueError, match="joint size"):
            fn(torch.zeros(2, 4, 96), torch.zeros(2, 3, 96), torch.zeros(96, 5), b2, sb, *rest, s_range=3)
        with pytest.raises(ValueError, match="joint size"):
            fn(torch.zeros(2, 4, 704), torch.zeros(2, 3, 704), torch.zeros(704, 5), b2, sb, *rest, s_range=3)
        with pytest.raises(ValueError, match="alphabet size"):
            fn(enc, pred, torch.zeros(64, 1), torch.zeros(1), sb, *rest, s_range=3)
        with pytest.raises(TypeError, match="float32"):
            fn(enc.double(), pred, W2, b2, sb, *rest, s_range=3)
        with pytest.raises(ValueError, match="s_range is required"):
            fn(enc, pred, W2, b2, sb, *rest)
        with pytest.raises(ValueError, match="s_range"):
            fn(enc, pred, W2, b2, sb, *rest, s_range=65)
        with pytest.raises(ValueError, match="s_range"):
            fn(enc, pred, W2, b2, sb, *rest, s_range=0)
        with pytest.raises(ValueError, match="s_begin"):
            fn(enc, pred, W2, b2, sb[:, :3], *rest, s_range=3)
        with pytest.raises(ValueError, match="s_begin"):
            fn(enc, pred, W2, b2, torch.zeros(2, 4, 2, dtype=torch.int32), *rest, s_range=3)
        with pytest.raises(TypeError, match="integer"):
            fn(enc, pred, W2, b2, sb.float(), *rest, s_range=3)
        with pytest.raises(ValueError, match="labels"):
            fn(enc, pred, W2, b2, sb, torch.ones(2, 3, dtype=torch.int32), *rest[1:], s_range=3)
        with pytest.raises(ValueError, match="topology"):
            fn(enc, pred, W2, b2, sb, *rest, topology="bogus", s_range=3)
        for lam in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match="fastemit_lambda"):
                fn(enc, pred, W2, b2, sb, *rest, fastemit_lambda=lam, s_range=3)
        with pytest.raises(ValueError, match="blank_label"):
            fn(enc, pred, W2, b2, sb, *rest, blank_label=5, s_range=3)


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_workspace_size(lib):
    n = _lib.pruned_joint_workspace_bytes(600, 5, 32, 640)
    slots = 32 * 600 * 5
    assert n % 256 == 0
    assert n >= slots * (36 + 640 * 4)                          # the lattice's 36 bytes per slot and one [J] array
    assert n < slots * (64 + 640 * 4) + 640 * 8192 * 4 + (1 << 16)  # and a J x 8192 block: no function of V or maxU
    assert _lib.pruned_joint_workspace_bytes(600, 5, 64, 640) > n and _lib.pruned_joint_workspace_bytes(601, 5, 32, 640) > n
    assert _lib.pruned_joint_workspace_bytes(600, 6, 32, 640) > n > _lib.pruned_joint_workspace_bytes(600, 5, 32, 576)
    out = ctypes.c_size_t(0)
    for args in ((0, 5, 32, 640), (600, 0, 32, 640), (600, 65, 32, 640), (600, 5, 0, 640), (1 << 20, 64, 32, 640),
                 (600, 5, 32, 0), (600, 5, 32, 96), (600, 5, 32, 704), (600, 5, 32, -64)):
        assert lib.get_rnnt_pruned_joint_workspace_size(*args, ctypes.byref(out)) == INVALID, args
    assert lib.get_rnnt_pruned_joint_workspace_size(600, 5, 32, 640, None) == INVALID
    assert lib.get_rnnt_pruned_joint_workspace_size(600, 64, 32, 64, ctypes.byref(out)) == 0


def test_argument_validation_needs_no_device(lib):
    fake = ctypes.c_void_p(256)  # never dereferenced: rejected before any launch
    o = _lib.make_options(0, 0, 10, 5)

    def call(enc=fake, pred=fake, W2=fake, b2=fake, sb=fake, labels=fake, ll=fake, il=fake, scale=None, J=64, V=28, B=4, S=5, topo=0,
             costs=fake, d_enc=fake, d_pred=fake, dW2=fake, db2=fake, ws=fake, opts=o, lam=0.0):
        return lib.compute_rnnt_joint_loss_pruned(enc, pred, W2, b2, sb, labels, ll, il, scale, J, V, B, S, topo, costs, d_enc, d_pred,
                                                  dW2, db2, ws, opts, lam)

    for name in ("enc", "pred", "W2", "b2", "sb", "labels", "ll", "il", "ws"):  # a NULL required pointer
        assert call(**{name: None}) == INVALID, name
    none = dict(d_enc=None, d_pred=None, dW2=None, db2=None)
    assert call(costs=None, **none) == INVALID           # nothing to compute
    for name in none:                                    # the gradients are all given or all NULL
        assert call(**{name: None}) == INVALID, name
        assert call(**{**none, name: fake}) == INVALID, name
    for J in (0, 32, 96, 704, -64):
        assert call(J=J) == INVALID, J
    for V in (0, 1, 8193):
        assert call(V=V) == INVALID, V
    assert call(B=0) == INVALID
    assert call(opts=_lib.make_options(0, 28, 10, 5)) == INVALID   # blank outside [0, V)
    assert call(opts=_lib.make_options(0, -1, 10, 5)) == INVALID
    assert call(S=0) == INVALID and call(S=65) == INVALID and call(S=-1) == INVALID
    assert call(topo=2) == INVALID and call(topo=-1) == INVALID
    assert call(opts=_lib.make_options(0, 0, 10, 0)) == INVALID     # maxU outside [1, 8192]
    assert call(opts=_lib.make_options(0, 0, 10, 8193)) == INVALID
    assert call(opts=_lib.make_options(0, 0, 1 << 20, 5), B=32, S=64) == INVALID  # B maxT S >= 2^31
    assert call(opts=_lib.make_options(0, 0, 1, 8192), B=1 << 18, S=1) == INVALID  # B maxU >= 2^31
    assert call(opts=_lib.make_options(0, 0, 10, 5, loc=_lib.RNNT_CPU)) == INVALID  # no CPU fallback in the library
    assert call(ws=ctypes.c_void_p(260)) == INVALID      # misaligned workspace
    for name in ("enc", "pred", "d_enc", "d_pred"):      # 16-byte rows
        assert call(**{name: ctypes.c_void_p(264)}) == INVALID, name
    for name in ("W2", "b2", "dW2", "db2", "costs", "scale", "sb"):
        assert call(**{name: ctypes.c_void_p(258)}) == INVALID, name
    for lam in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
        assert call(lam=lam) == INVALID, lam
