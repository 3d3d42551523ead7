"""CPU tests of FastEmit regularisation (include/rnnt.h compute_rnnt_loss_fastemit): the float64 restatement the GPU tests
compare against (tests/fastemit_cases.py) is checked against an independent derivation -- torch float64 autograd of the plain
transducer cost on  lp + lambda mask_label (lp - lp.detach())  (a straight-through term: the value of lp is unchanged, the gradient
of its label entries is scaled by 1 + lambda) -- and the ABI / Python surface of the feature."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from oracle import rnnt_oracle as orc
from rnnt_speech_recognition_amd import _lib
from tests import fastemit_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("compute_rnnt_loss_fastemit", "compute_rnnt_joint_loss_bwd_fastemit", "compute_rnnt_joint_net_loss_bwd_fastemit")


def _torch_cost(lp, labels, blank=0):
    """-ln P of one utterance from log-probabilities lp [T, U, V] (float64 tensor), differentiable."""
    T, U, _ = lp.shape
    neg = torch.tensor(-1.0e300, dtype=torch.float64)
    a = [[None] * U for _ in range(T)]
    for t in range(T):
        for u in range(U):
            if t == 0 and u == 0:
                a[t][u] = torch.zeros((), dtype=torch.float64)
                continue
            up = a[t - 1][u] + lp[t - 1, u, blank] if t > 0 else neg
            lf = a[t][u - 1] + lp[t, u - 1, int(labels[u - 1])] if u > 0 else neg
            a[t][u] = torch.logaddexp(up, lf)
    return -(a[T - 1][U - 1] + lp[T - 1, U - 1, blank])


def _straight_through(x, labels, lam, blank=0):
    x = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    lp = torch.log_softmax(x, dim=-1)
    T, U, V = lp.shape
    mask = torch.zeros_like(lp)
    for u in range(U - 1):
        mask[:, u, int(labels[u])] = 1.0
    cost = _torch_cost(lp + lam * mask * (lp - lp.detach()), labels, blank)
    cost.backward()
    return float(cost.detach()), x.grad.numpy()


@pytest.mark.parametrize("T,U,V,lam,blank", [(5, 4, 6, 0.5, 0), (4, 3, 5, 1.0, 2), (6, 1, 4, 0.5, 0), (1, 4, 5, 0.25, 0), (3, 3, 3, 0.01, 1)])
def test_restatement_equals_straight_through_autograd(T, U, V, lam, blank):
    rng = np.random.default_rng(T * 100 + U * 10 + V)
    x = rng.normal(size=(T, U, V)) * 2.0
    labels = [int(v) for v in rng.integers(0, V, size=max(U - 1, 0)) if True]
    labels = [(v + 1) % V if v == blank else v for v in labels]
    c_ref, g_ref = _straight_through(x, labels, lam, blank)
    c, g = fc.utterance(x, np.asarray(labels, np.int64), lam, blank)
    assert abs(c - c_ref) <= 1e-10
    assert np.abs(g - g_ref).max() <= 1e-10


def test_every_cell_sums_to_zero_and_lambda_zero_is_the_oracle():
    acts, labels, il, ll = fc.op_case(3, 9, 5, 28, seed=1)
    scale = np.array([0.5, 1.0, 2.0])
    for lam in (0.0, 0.5, 1.0):
        _, g = fc.loss_and_grad(acts, labels, il, ll, lam, scale)
        assert np.abs(g.sum(-1)).max() <= 1e-12
        for b in range(3):
            assert not g[b, il[b]:].any() and not g[b, :, ll[b] + 1:].any()
    c0, g0 = fc.loss_and_grad(acts, labels, il, ll, 0.0)
    c_ref, g_ref = orc.rnnt_loss_and_grad(acts, labels, il, ll)
    assert np.abs(c0 - c_ref).max() <= 1e-12 and np.abs(g0 - g_ref).max() <= 1e-12
    # the costs do not depend on lambda; the gradients are affine in it
    c1, g1 = fc.loss_and_grad(acts, labels, il, ll, 1.0)
    ch, gh = fc.loss_and_grad(acts, labels, il, ll, 0.5)
    assert (c1 == c0).all() and (ch == c0).all()
    assert np.abs(gh - 0.5 * (g0 + g1)).max() <= 1e-12
    assert np.abs(g1 - g0).max() > 1e-2  # ... and it does something


def test_joint_restatement_at_lambda_zero_is_the_oracle():
    case = fc.joint_case(2, 6, 4, 8, 16, 12, seed=2)
    ref = orc.joint_loss_and_grads(*case, cost_scale=np.array([1.0, 0.5]))
    out = fc.joint_loss_and_grads(*case, 0.0, cost_scale=np.array([1.0, 0.5]))
    for k in fc.GRAD_KEYS + ("costs",):
        assert np.abs(out[k] - ref[k]).max() <= 1e-12, k


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnnt.h")).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(([^;{]*)\)\s*;", text)}


def test_header_binding_and_exports_agree():
    decl = _declared()
    pkg.build()
    lib = _lib.load()
    for name in NEW:
        assert name in decl and name in _lib.SYMBOLS, name
        assert re.search(r"float\s+fastemit_lambda\s*$", decl[name].strip()), name  # the trailing argument
        fn = getattr(lib, name)
        assert ctypes.cast(fn, ctypes.c_void_p).value
        assert fn.argtypes[-1] is ctypes.c_float and fn.restype is ctypes.c_int
        # the rest of the signature is the existing entry point's
        base = {"compute_rnnt_loss_fastemit": "compute_rnnt_loss_flags"}.get(name, name[: -len("_fastemit")])
        assert list(fn.argtypes[:-1]) == list(getattr(lib, base).argtypes), name
        strip = lambda s: re.sub(r"\s+", " ", s).strip()
        assert strip(decl[name]).startswith(strip(decl[base])), name
    assert len(decl) == 66 == len(_lib.SYMBOLS)


def test_out_of_range_lambda_is_refused_before_any_device_work():
    pkg.build()
    lib = _lib.load()
    fake = ctypes.c_void_p(256)  # never dereferenced
    o = _lib.make_options(0, 0, 10, 5)
    for lam in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
        assert lib.compute_rnnt_loss_fastemit(fake, fake, fake, fake, fake, None, 28, 4, fake, fake, o, 0, lam) == 2
        assert lib.compute_rnnt_joint_loss_bwd_fastemit(*([fake] * 7), None, 64, 28, 4, fake, fake, fake, fake, 0, fake, o, lam) == 2
        assert lib.compute_rnnt_joint_net_loss_bwd_fastemit(*([fake] * 9), None, 32, 64, 28, 4, *([fake] * 6), 0, fake, o, lam) == 2
    assert lib.compute_rnnt_loss_fastemit(fake, fake, fake, fake, fake, None, 28, 4, fake, fake, o, 0x2, 0.5) == 2  # unknown flag bit


@pytest.mark.parametrize("lam", [-0.1, 1.5, float("nan"), float("inf")])
def test_python_surface_raises_on_out_of_range_lambda(lam):
    x = torch.zeros(1, 2, 2, 4)
    lab, one, two = torch.ones(1, 1, dtype=torch.int32), torch.tensor([1]), torch.tensor([2])
    with pytest.raises(ValueError, match="fastemit_lambda"):
        pkg.rnnt_loss(x, lab, two, one, fastemit_lambda=lam)
    with pytest.raises(ValueError, match="fastemit_lambda"):
        pkg.rnnt_loss_and_grad(x, lab, two, one, fastemit_lambda=lam)
    with pytest.raises(ValueError, match="fastemit_lambda"):
        pkg.RNNTLoss(fastemit_lambda=lam)
    with pytest.raises(ValueError, match="fastemit_lambda"):
        pkg.JointLoss(8, 64, 28, fastemit_lambda=lam)
    e = torch.zeros(1, 2, 8)
    with pytest.raises(ValueError, match="fastemit_lambda"):
        pkg.rnnt_joint_loss(e, e, torch.zeros(8, 64), torch.zeros(64), torch.zeros(64, 28), torch.zeros(28), lab, two, one,
                            fastemit_lambda=lam)
    hp = pkg.HParams(vocab_size=28, mel_bins=8, downsample_factor=3, embedding_size=16, encoder_layers=2, encoder_size=48,
                     projection_size=32, time_reduction_index=0, time_reduction_factor=2, pred_net_layers=1, pred_net_size=48,
                     joint_net_size=64)
    with pytest.raises(ValueError, match="fastemit_lambda"):
        pkg.Transducer(hp, fastemit_lambda=lam)


def test_keyword_reaches_the_joint_loss_of_the_model():
    hp = pkg.HParams(vocab_size=28, mel_bins=8, downsample_factor=3, embedding_size=16, encoder_layers=2, encoder_size=48,
                     projection_size=32, time_reduction_index=0, time_reduction_factor=2, pred_net_layers=1, pred_net_size=48,
                     joint_net_size=64)
    assert pkg.Transducer(hp, fastemit_lambda=0.01).joint.fastemit_lambda == 0.01
    assert pkg.Transducer(hp).joint.fastemit_lambda == 0.0 and pkg.RNNTLoss().fastemit_lambda == 0.0
