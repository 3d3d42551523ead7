"""CPU tests of the simple (additive joiner) transducer loss (include/rnnt_simple.h): they pin the float64 restatement of
tests/simple_cases.py against the full-lattice oracles and the lattices' frame identities, the torch mirror and the plumbing of
rnnt_speech_recognition_amd.simple against the restatement, and check what needs no device: the ABI and the argument validation."""
import ctypes

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from oracle import rnnt_oracle as orc
from rnnt_speech_recognition_amd import _lib, simple
from tests import fastemit_cases as fc
from tests import modified_cases as mc
from tests import simple_cases as sc

INVALID = 2  # RNNT_STATUS_INVALID_VALUE


@pytest.fixture(scope="module")
def lib():
    pkg.build()
    return _lib.load_simple()


def _t(*arrays):
    return [torch.as_tensor(a) for a in arrays]


# ---- the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
def test_without_scales_it_is_the_full_lattice_op_on_the_sum(topology):
    """am[:, :, None] + lm[:, None] through the existing float64 oracles: the same costs, and their gradient summed over u and over t."""
    am, lm, labels, il, ll = sc.case(3, 9, 6, 7, seed=2)
    am, lm = np.nan_to_num(am), np.nan_to_num(lm)
    acts = am[:, :, None, :].astype(np.float64) + lm[:, None, :, :]
    c_ref, g_ref = orc.rnnt_loss_and_grad(acts, labels, il, ll) if topology == "standard" else mc.loss_and_grad(acts, labels, il, ll)
    r = sc.loss_and_grad(am, lm, labels, il, ll, topology=topology)
    assert np.isfinite(c_ref).all()
    assert np.abs(r["costs"] - c_ref).max() <= 1e-10
    assert np.abs(r["g_am"] - g_ref.sum(2)).max() <= 1e-10 and np.abs(r["g_lm"] - g_ref.sum(1)).max() <= 1e-10
    assert np.abs(r["g_am"]).max() > 1e-2 and np.abs(r["g_lm"]).max() > 1e-2
    c, occ, g_am, g_lm = pkg.rnnt_loss_simple_and_grad(*_t(am, lm, labels, il, ll), topology=topology)
    assert np.abs(c.numpy() - c_ref).max() <= 1e-10
    assert np.abs(g_am.numpy() - g_ref.sum(2)).max() <= 1e-10 and np.abs(g_lm.numpy() - g_ref.sum(1)).max() <= 1e-10


@pytest.mark.parametrize("l,a", sc.SCALES)
def test_frame_identities(l, a):
    """Every path of the standard lattice leaves every frame by exactly one blank edge: sum_u e_b(t, u) = 1.  Every path of the
    modified lattice takes exactly one edge per frame: sum_u occ(t, u) = 1."""
    am, lm, labels, il, ll = sc.case(4, 11, 6, 5, seed=3)
    for topology in sc.TOPOLOGIES:
        r = sc.loss_and_grad(am, lm, labels, il, ll, l=l, a=a, topology=topology)
        for b in range(4):
            if not np.isfinite(r["costs"][b]):
                assert topology == "modified" and ll[b] > il[b]
                continue
            rows = (r["e_b"] if topology == "standard" else r["occ"])[b, :il[b]].sum(1)
            assert np.abs(rows - 1.0).max() <= 1e-12
            assert not r["occ"][b, il[b]:].any() and not r["occ"][b, :, ll[b] + 1:].any()


def test_restatement_gradients_match_finite_differences():
    rng = np.random.default_rng(1)
    am, lm, y = rng.normal(size=(4, 5)), rng.normal(size=(3, 5)), [2, 4]
    for topology in sc.TOPOLOGIES:
        for l, a in ((0.0, 0.0), (0.25, 0.25)):
            _, _, _, g_am, g_lm = sc.utterance(am, lm, y, 0, l, a, topology)
            h = 1e-5
            for x, g in ((am, g_am), (lm, g_lm)):
                for idx in np.ndindex(*x.shape):
                    keep = x[idx]
                    x[idx] = keep + h
                    cp = sc.utterance(am, lm, y, 0, l, a, topology)[0]
                    x[idx] = keep - h
                    cm = sc.utterance(am, lm, y, 0, l, a, topology)[0]
                    x[idx] = keep
                    assert abs((cp - cm) / (2 * h) - g[idx]) <= 1e-7


def test_more_labels_than_frames():
    am, lm, labels, il, ll = sc.case(2, 3, 6, 5, seed=4, ragged=False)
    r = sc.loss_and_grad(am, lm, labels, il, ll, topology="modified")
    assert (r["costs"] == np.inf).all() and not r["occ"].any() and not r["g_am"].any() and not r["g_lm"].any()
    c, occ, g_am, g_lm = pkg.rnnt_loss_simple_and_grad(*_t(am, lm, labels, il, ll), topology="modified")
    assert (c == float("inf")).all() and not occ.any() and not g_am.any() and not g_lm.any()
    assert np.isfinite(sc.loss_and_grad(am, lm, labels, il, ll, topology="standard")["costs"]).all()


# ---- the mirror ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
@pytest.mark.parametrize("l,a", sc.SCALES)
def test_mirror_is_the_restatement(topology, l, a):
    for seed, blank, shape in ((10, 0, (4, 9, 6, 7)), (11, 3, (3, 5, 1, 4)), (12, 1, (3, 1, 3, 2))):
        am, lm, labels, il, ll = sc.case(*shape, seed=seed, blank=blank)
        scale = np.linspace(-1.5, 2.0, shape[0])
        r = sc.loss_and_grad(am, lm, labels, il, ll, blank, l, a, topology, cost_scale=scale)
        c, occ, g_am, g_lm = simple._mirror(*_t(am, lm, labels, il, ll), blank, l, a, topology, cost_scale=scale)
        fin = np.isfinite(r["costs"])
        assert np.array_equal(c.numpy()[~fin], r["costs"][~fin]) and np.abs(c.numpy()[fin] - r["costs"][fin]).max(initial=0) <= 1e-10
        assert np.abs(occ.numpy() - r["occ"]).max() <= 1e-10
        assert np.abs(g_am.numpy() - r["g_am"]).max() <= 1e-10 and np.abs(g_lm.numpy() - r["g_lm"]).max() <= 1e-10
        c2, occ2 = pkg.rnnt_loss_simple(*_t(am, lm, labels, il, ll), blank_label=blank, lm_only_scale=l, am_only_scale=a, topology=topology)
        assert torch.equal(c2, c) and torch.equal(occ2, occ) and not occ2.requires_grad


@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
def test_mirror_autograd_matches_finite_differences(topology):
    am, lm, labels, il, ll = sc.case(2, 5, 3, 4, seed=20)
    am, lm = np.nan_to_num(am).astype(np.float64), np.nan_to_num(lm).astype(np.float64)
    weights = torch.tensor([0.5, -1.5], dtype=torch.float64)
    rest = _t(labels, il, ll)

    def value(am_, lm_):
        return (weights * pkg.rnnt_loss_simple(am_, lm_, *rest, lm_only_scale=0.25, am_only_scale=0.25, topology=topology)[0]).sum()

    x, y = torch.tensor(am, requires_grad=True), torch.tensor(lm, requires_grad=True)
    value(x, y).backward()
    assert x.grad.abs().max() > 1e-2 and y.grad.abs().max() > 1e-2
    h = 1e-5
    for arr, grad, which in ((am, x.grad, 0), (lm, y.grad, 1)):
        for idx in np.ndindex(*arr.shape):
            if (which == 0 and idx[1] >= il[idx[0]]) or (which == 1 and idx[1] > ll[idx[0]]):
                assert grad[idx] == 0
                continue
            keep = arr[idx]
            arr[idx] = keep + h
            vp = value(torch.tensor(am), torch.tensor(lm)).item()
            arr[idx] = keep - h
            vm = value(torch.tensor(am), torch.tensor(lm)).item()
            arr[idx] = keep
            assert abs((vp - vm) / (2 * h) - grad[idx].item()) <= 1e-7


@pytest.mark.parametrize("what,value", [("T", 0), ("T", 10), ("L", -1), ("L", 6)])
def test_mirror_out_of_range_lengths(what, value):
    am, lm, labels, il, ll = sc.case(3, 9, 6, 7, seed=30, ragged=False)
    il_bad, ll_bad = il.copy(), ll.copy()
    (il_bad if what == "T" else ll_bad)[1] = value
    c, occ, g_am, g_lm = pkg.rnnt_loss_simple_and_grad(*_t(am, lm, labels, il_bad, ll_bad))
    Tc, Lc = int(np.clip(il_bad[1], 1, 9)), int(np.clip(ll_bad[1], 0, 5))
    assert torch.isnan(c[1]) and torch.isnan(occ[1, :Tc, :Lc + 1]).all() and torch.isnan(g_am[1, :Tc]).all() and torch.isnan(g_lm[1, :Lc + 1]).all()
    assert not occ[1, Tc:].any() and not occ[1, :, Lc + 1:].any() and not g_am[1, Tc:].any() and not g_lm[1, Lc + 1:].any()
    r = sc.loss_and_grad(am, lm, labels, il, ll)
    assert np.abs(c.numpy()[[0, 2]] - r["costs"][[0, 2]]).max() <= 1e-10


@pytest.mark.parametrize("topology", sc.TOPOLOGIES)
def test_two_pass_with_a_full_band_is_the_full_lattice_loss(topology):
    """s_range >= U: every band begins at 0 and holds the whole lattice, so the pruned cost is the joint's full-lattice cost."""
    B, T, U, J, V = 2, 8, 5, 6, 7
    enc, pred, _, _, W2, b2, labels, il, ll = fc.joint_case(B, T, U, J, J, V, seed=40)
    rng = np.random.default_rng(41)
    am, lm = rng.normal(size=(B, T, V)).astype(np.float32), rng.normal(size=(B, U, V)).astype(np.float32)
    W, bias = torch.tensor(W2), torch.tensor(b2)
    joint = lambda a, p: torch.tanh(a + p) @ W + bias  # noqa: E731
    for S in (U, U + 3):
        sc_, pr, sb = pkg.rnnt_loss_two_pass(*_t(am, lm, enc, pred), joint, *_t(labels, il, ll), S, topology=topology)
        assert sb.dtype == torch.int32 and tuple(sb.shape) == (B, T) and not sb.any()
        full = (np.tanh(enc[:, :, None, :] + pred[:, None, :, :]) @ W2 + b2).astype(np.float64)
        c_ref, _ = orc.rnnt_loss_and_grad(full, labels, il, ll) if topology == "standard" else mc.loss_and_grad(full, labels, il, ll)
        assert np.abs(pr.numpy() - c_ref).max() <= 1e-5 * np.abs(c_ref).max()  # (the joint runs in float32)
        assert np.abs(sc_.numpy() - sc.loss_and_grad(am, lm, labels, il, ll, topology=topology)["costs"]).max() <= 1e-10


def test_two_pass_is_differentiable_in_all_four_inputs():
    B, T, U, J, V, S = 2, 8, 5, 6, 7, 2
    enc, pred, _, _, W2, b2, labels, il, ll = fc.joint_case(B, T, U, J, J, V, seed=42)
    rng = np.random.default_rng(43)
    leaves = [torch.tensor(x, requires_grad=True) for x in (rng.normal(size=(B, T, V)).astype(np.float32),
                                                            rng.normal(size=(B, U, V)).astype(np.float32), enc, pred)]
    W, bias = torch.tensor(W2), torch.tensor(b2)
    s, p, sb = pkg.rnnt_loss_two_pass(*leaves, lambda a, q: torch.tanh(a + q) @ W + bias, *_t(labels, il, ll), S,
                                      lm_only_scale=0.25, am_only_scale=0.0)
    (0.5 * s.sum() + p.sum()).backward()
    assert all(x.grad is not None and x.grad.abs().max() > 1e-3 for x in leaves)
    assert (sb[:, 0] == 0).all() and (sb.diff(dim=1) >= 0).all()


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_workspace_size(lib):
    n = _lib.simple_workspace_bytes(600, 150, 32)
    assert n % 256 == 0
    assert n >= 32 * 600 * 150 * (8 + 8 + 8 + 4 + 8)  # {lpb, lpl}, alpha, beta, Z and {e_b, e_l} per cell
    assert n < 32 * (600 + 150) * 192 * 32              # no function of V: the interface has none
    assert _lib.simple_workspace_bytes(600, 150, 64) > n and _lib.simple_workspace_bytes(601, 150, 32) > n
    assert _lib.simple_workspace_bytes(600, 151, 32) > n
    out = ctypes.c_size_t(0)
    for args in ((0, 5, 32), (600, 0, 32), (600, 8193, 32), (600, 5, 0), (1 << 20, 64, 32)):
        assert lib.get_rnnt_simple_workspace_size(*args, ctypes.byref(out)) == INVALID, args
    assert lib.get_rnnt_simple_workspace_size(600, 5, 32, None) == INVALID
    assert lib.get_rnnt_simple_workspace_size(4, 8192, 2, ctypes.byref(out)) == 0


def test_argument_validation_needs_no_device(lib):
    fake = ctypes.c_void_p(256)  # never dereferenced: rejected before any launch
    o = _lib.make_options(0, 0, 10, 5)

    def call(am=fake, lm=fake, g_am=fake, g_lm=fake, occ=fake, labels=fake, ll=fake, il=fake, scale=None, V=28, B=4, topo=0,
             l=0.0, a=0.0, costs=fake, ws=fake, opts=o):
        return lib.compute_rnnt_loss_simple(am, lm, g_am, g_lm, occ, labels, ll, il, scale, V, B, topo, l, a, costs, ws, opts)

    for name in ("am", "lm", "labels", "ll", "il", "ws"):  # a NULL required pointer
        assert call(**{name: None}) == INVALID, name
    assert call(g_am=None, g_lm=None, occ=None, costs=None) == INVALID  # nothing to compute
    assert call(g_am=None) == INVALID and call(g_lm=None) == INVALID      # exactly one of the two gradient pointers
    assert call(V=1) == INVALID and call(V=0) == INVALID                  # alphabet_size < 2
    assert call(B=0) == INVALID
    assert call(opts=_lib.make_options(0, 28, 10, 5)) == INVALID          # blank outside [0, V)
    assert call(opts=_lib.make_options(0, -1, 10, 5)) == INVALID
    assert call(topo=2) == INVALID and call(topo=-1) == INVALID
    assert call(opts=_lib.make_options(0, 0, 10, 0)) == INVALID           # maxU outside [1, 8192]
    assert call(opts=_lib.make_options(0, 0, 10, 8193)) == INVALID
    assert call(opts=_lib.make_options(0, 0, 1 << 20, 64), B=32) == INVALID  # B maxT maxU >= 2^31
    assert call(opts=_lib.make_options(0, 0, 10, 5, loc=_lib.RNNT_CPU)) == INVALID  # no CPU fallback in the library
    assert call(ws=ctypes.c_void_p(260)) == INVALID                       # misaligned workspace
    for bad in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
        assert call(l=bad) == INVALID and call(a=bad) == INVALID, bad
    assert call(l=0.75, a=0.5) == INVALID                                 # the sum outside [0, 1]


def test_python_argument_errors():
    am, lm = torch.zeros(2, 4, 5), torch.zeros(2, 3, 5)
    rest = (torch.ones(2, 2, dtype=torch.int32), torch.tensor([4, 4]), torch.tensor([2, 2]))
    for fn in (pkg.rnnt_loss_simple, pkg.rnnt_loss_simple_and_grad):
        with pytest.raises(ValueError, match="am must be"):
            fn(am[0], lm, *rest)
        with pytest.raises(ValueError, match="agree"):
            fn(am, torch.zeros(2, 3, 6), *rest)
        with pytest.raises(ValueError, match="labels"):
            fn(am, torch.zeros(2, 4, 5), *rest)
        with pytest.raises(TypeError, match="float32"):
            fn(am.half(), lm.half(), *rest)
        with pytest.raises(ValueError, match="topology"):
            fn(am, lm, *rest, topology="bogus")
        with pytest.raises(ValueError, match="blank_label"):
            fn(am, lm, *rest, blank_label=5)
        for l, a in ((-0.1, 0.0), (0.0, 1.5), (float("nan"), 0.0), (0.75, 0.5)):
            with pytest.raises(ValueError, match="only_scale"):
                fn(am, lm, *rest, lm_only_scale=l, am_only_scale=a)
