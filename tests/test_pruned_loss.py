"""CPU tests of the pruned transducer loss (include/rnnt_pruned.h): they pin the float64 restatement of tests/pruned_cases.py
against the path sum, finite differences and the full-lattice oracles, the torch mirror and the plumbing of
rnnt_speech_recognition_amd.pruning against the restatement, and check what needs no device: the ABI and the argument validation."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from oracle import rnnt_oracle as orc
from rnnt_speech_recognition_amd import _lib, pruning
from tests import fastemit_cases as fc
from tests import modified_cases as mc
from tests import pruned_cases as pc

INVALID = 2  # RNNT_STATUS_INVALID_VALUE


@pytest.fixture(scope="module")
def lib():
    pkg.build()
    return _lib.load_pruned()


# ---- the restatement ----------------------------------------------------------------------------------------------------
def _tiny_bands(T, L, S):
    """Every non-decreasing sb from 0 to max(0, L + 1 - S) with steps <= S, so connected and disconnected bands both occur
    (capped: the first 12 in lexicographic order plus a decreasing one)."""
    hi = max(0, L + 1 - S)
    out = []
    for mid in itertools.product(range(hi + 1), repeat=T - 2):
        sb = (0,) + mid + (hi,)
        if all(0 <= b - a <= S for a, b in zip(sb, sb[1:])):
            out.append(sb)
    return out[:12] + [tuple(reversed(out[-1]))]


@pytest.mark.parametrize("topology", pc.TOPOLOGIES)
@pytest.mark.parametrize("T,L,S", [(3, 0, 1), (3, 1, 1), (4, 2, 2), (5, 3, 2), (6, 3, 3), (4, 3, 1), (5, 2, 3), (6, 1, 2)])
def test_cost_is_the_sum_over_all_paths(topology, T, L, S):
    rng = np.random.default_rng(T * 100 + L * 10 + S)
    x = rng.normal(size=(T, S, 4))
    y = rng.integers(1, 4, size=max(L, 1))
    seen = set()
    for sb in _tiny_bands(T, L, S):
        cost, g = pc.utterance(x, sb, y, T, L, topology=topology)
        brute = pc.brute_force_cost(x, sb, y, T, L, topology=topology)
        seen.add(bool(np.isfinite(brute)))
        if np.isfinite(brute):
            assert abs(cost - brute) <= 1e-12
        else:
            assert cost == np.inf and not g.any()
    assert True in seen or L > 0


@pytest.mark.parametrize("topology", pc.TOPOLOGIES)
def test_a_step_of_the_band_width_disconnects(topology):
    rng = np.random.default_rng(3)
    T, L, S = 4, 3, 2
    x, y = rng.normal(size=(T, S, 4)), rng.integers(1, 4, size=L)
    sb = (0, 0, 2, 2) if topology == "standard" else (0, 0, 3, 2)  # (modified: a diagonal step reaches one column further)
    cost, g = pc.utterance(x, sb, y, T, L, lam=0.5, topology=topology)
    assert cost == np.inf and g.shape == x.shape and not g.any()
    assert pc.brute_force_cost(x, sb, y, T, L, topology=topology) == np.inf


@pytest.mark.parametrize("topology", pc.TOPOLOGIES)
def test_gradients_match_finite_differences(topology):
    rng = np.random.default_rng(1)
    T, L, S = 5, 3, 2
    x, y, sb = rng.normal(size=(T, S, 4)), rng.integers(1, 4, size=L), (0, 0, 1, 1, 2)
    _, g = pc.utterance(x, sb, y, T, L, topology=topology)
    h = 1e-5
    num = np.zeros_like(x)
    for idx in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[idx] += h
        xm[idx] -= h
        num[idx] = (pc.utterance(xp, sb, y, T, L, topology=topology)[0] - pc.utterance(xm, sb, y, T, L, topology=topology)[0]) / (2 * h)
    assert np.abs(num - g).max() <= 1e-7
    assert np.abs(g).max() > 1e-2


def test_the_full_band_is_the_full_lattice():
    acts, labels, il, ll = fc.op_case(3, 9, 6, 7, seed=2)
    sb = np.zeros(acts.shape[:2], np.int32)
    c, g = pc.loss_and_grad(acts, sb, labels, il, ll, topology="standard")
    c_ref, g_ref = orc.rnnt_loss_and_grad(acts, labels, il, ll)
    assert np.abs(c - c_ref).max() <= 1e-12 and np.abs(g - g_ref).max() <= 1e-12
    c, g = pc.loss_and_grad(acts, sb, labels, il, ll, lam=0.01, topology="standard")
    c_ref, g_ref = fc.loss_and_grad(acts, labels, il, ll, 0.01)
    assert np.abs(c - c_ref).max() <= 1e-12 and np.abs(g - g_ref).max() <= 1e-12
    c, g = pc.loss_and_grad(acts, sb, labels, il, ll, lam=0.01, topology="modified")
    c_ref, g_ref = mc.loss_and_grad(acts, labels, il, ll, 0.01)
    assert np.abs(c - c_ref).max() <= 1e-12 and np.abs(g - g_ref).max() <= 1e-12


@pytest.mark.parametrize("topology", pc.TOPOLOGIES)
def test_restricting_the_band_never_lowers_the_cost(topology):
    full, labels, il, ll = fc.op_case(2, 10, 7, 5, seed=4)
    rng = np.random.default_rng(4)
    c_full, _ = pc.loss_and_grad(full, np.zeros((2, 10), np.int32), labels, il, ll, topology=topology)
    last = c_full
    for S in (6, 4, 3, 2):
        sb = pc.staircase_ranges(rng, 2, 10, S, il, ll, steps=[0, 1])
        c, _ = pc.loss_and_grad(pc.gather_band(full, sb, S), sb, labels, il, ll, topology=topology)
        assert (c >= c_full - 1e-12).all()
        last = c
    assert (last > c_full).any()


@pytest.mark.parametrize("topology", pc.TOPOLOGIES)
@pytest.mark.parametrize("lam", [0.0, 0.01, 1.0])
def test_row_sums(topology, lam):
    """sum_v grads[t,s,v] = cs ((occ + lambda e_l) - e_b - (1 + lambda) e_l) = 0 for every lambda: FastEmit (section 8k) scales the
    label edge's gradient on both sides of the softmax, so a row still sums to zero; the costs do not depend on lambda."""
    acts, sb, labels, il, ll = pc.band_case(2, 8, 5, 3, 6, seed=5)
    c, g = pc.loss_and_grad(acts, sb, labels, il, ll, lam=lam, topology=topology)
    c0, g0 = pc.loss_and_grad(acts, sb, labels, il, ll, topology=topology)
    assert np.isfinite(c).all() and np.array_equal(c, c0)
    assert np.abs(g.sum(-1)).max() <= 1e-14
    assert not g[~pc.present_mask(sb, il, ll, 3)].any()
    assert lam == 0.0 or np.abs(g - g0).max() > 1e-4 * lam


# ---- the torch mirror and the plumbing ----------------------------------------------------------------------------------
def _t(*arrays):
    return [torch.as_tensor(np.asarray(a)) for a in arrays]


@pytest.mark.parametrize("topology", pc.TOPOLOGIES)
def test_mirror_is_the_restatement(topology):
    for S, blank, seed in ((1, 0, 6), (3, 2, 7), (5, 5, 8)):
        acts, sb, labels, il, ll = pc.band_case(4, 9, 6, S, 6, seed=seed, blank=blank)
        sb[3, 2:5] = [7, -2, 2 ** 31 - 1]  # hostile values as well
        acts = pc.poison_absent(np.nan_to_num(acts), sb, il, ll)
        c_ref, g_ref = pc.loss_and_grad(acts, sb, labels, il, ll, lam=0.25, blank=blank, topology=topology)
        c, g = pkg.rnnt_loss_pruned_and_grad(*_t(acts, sb, labels, il, ll), blank_label=blank, fastemit_lambda=0.25, topology=topology)
        assert c.dtype == torch.float64 and g.dtype == torch.float64
        fin = np.isfinite(c_ref)
        assert np.array_equal(c.numpy()[~fin], c_ref[~fin])
        assert np.abs(c.numpy()[fin] - c_ref[fin]).max(initial=0.0) <= 1e-10 and np.abs(g.numpy() - g_ref).max() <= 1e-10
        # autograd through the mirror, weighted; k2's [B, T, S] ranges
        w = np.where(fin, np.linspace(-1.0, 2.0, 4), 0.0)
        x = torch.tensor(acts, requires_grad=True)
        ranges = torch.as_tensor(sb.astype(np.int64))[:, :, None] + torch.arange(S)
        costs = pkg.rnnt_loss_pruned(x, ranges, *_t(labels, il, ll), blank_label=blank, fastemit_lambda=0.25, topology=topology)
        (costs[torch.as_tensor(fin)] * torch.as_tensor(w[fin])).sum().backward()
        assert x.grad.dtype == torch.float32
        assert np.abs(x.grad.numpy() - g_ref * w[:, None, None, None]).max() <= 1e-6


def _check_ranges(sb, il, ll, S):
    B, T = sb.shape
    for b in range(B):
        Tb, hi = int(il[b]), max(0, int(ll[b]) + 1 - S)
        r = sb[b, :Tb].astype(np.int64)
        assert r[0] == (0 if Tb > 1 else hi) and r[-1] == hi
        assert (np.diff(r) >= 0).all() and (r >= 0).all() and (r <= hi).all()
        # consecutive bands overlap wherever the rule can arrange it: step 4 raises sb[t] for t >= 1 and leaves sb[0] = 0 alone,
        # so the step out of frame 0 is whatever the occupancies ask for
        assert (np.diff(r[1:]) <= max(S - 1, 0)).all()
        assert (sb[b, Tb:] == hi).all()


@pytest.mark.parametrize("S", [1, 2, 3, 5])
def test_prune_ranges_properties(S):
    rng = np.random.default_rng(S)
    B, T, U = 5, 14, 9
    occ = rng.random((B, T, U)) ** 4
    il = np.array([14, 9, 1, 14, 2], np.int32)
    ll = np.array([8, 3, 0, 1, 8], np.int32)
    sb = pkg.prune_ranges(*_t(occ, il, ll), S)
    assert sb.dtype == torch.int32 and tuple(sb.shape) == (B, T)
    _check_ranges(sb.numpy(), il, ll, S)
    # the rule itself, step by step, for one utterance
    b, Tb, hi = 0, 14, max(0, 8 + 1 - S)
    want = np.array([max(range(hi + 1), key=lambda s0: (occ[b, t, s0:s0 + S].sum(), -s0)) for t in range(Tb)])
    want[0], want[Tb - 1] = 0, hi
    want = np.maximum.accumulate(want)
    for t in range(Tb - 2, 0, -1):
        want[t] = max(want[t], want[t + 1] - (S - 1))
    assert np.array_equal(sb.numpy()[b, :Tb], want)


@pytest.mark.parametrize("S", [2, 3, 5])
def test_prune_ranges_keeps_a_staircase_path_inside_the_band(S):
    rng = np.random.default_rng(10 + S)
    B, T, L = 3, 20, 11
    U = L + 1
    il, ll = np.array([20, 13, 20], np.int32), np.array([11, 11, 4], np.int32)
    occ = np.zeros((B, T, U))
    cells = []
    for b in range(B):
        Tb, Lb = int(il[b]), int(ll[b])
        emit = np.zeros(Tb, np.int64)  # labels emitted on frame t: at most S - 1, L_b in all
        for _ in range(Lb):
            emit[rng.choice(np.nonzero(emit < S - 1)[0])] += 1
        u, path = 0, []
        for t in range(Tb):
            for _ in range(emit[t] + 1):  # the cells the path visits on this frame
                path.append((t, u))
                u += 1
            u -= 1
        assert u == Lb
        for t, u in path:
            occ[b, t, u] = 1.0
        cells.append(path)
    sb = pkg.prune_ranges(*_t(occ, il, ll), S).numpy()
    _check_ranges(sb, il, ll, S)
    for b in range(B):
        for t, u in cells[b]:
            assert sb[b, t] <= u < sb[b, t] + S, (b, t, u, sb[b, t])


def test_prune_joint_inputs():
    B, T, U, J, S = 2, 5, 4, 3, 3
    enc = torch.arange(B * T * J, dtype=torch.float32).reshape(B, T, J)
    pred = torch.arange(B * U * J, dtype=torch.float32).reshape(B, U, J).requires_grad_()
    sb = torch.tensor([[0, 1, 2, 3, -5], [2 ** 31 - 1, 0, 0, 1, 1]], dtype=torch.int32)
    a, p = pkg.prune_joint_inputs(enc, pred, sb, S)
    assert tuple(a.shape) == (B, T, 1, J) and tuple(p.shape) == (B, T, S, J)
    assert torch.equal(a[:, :, 0], enc)
    for b in range(B):
        for t in range(T):
            for s in range(S):
                u = min(max(int(sb[b, t]) + s, 0), U - 1)  # the clamp
                assert torch.equal(p[b, t, s], pred[b, u])
    p.sum().backward()
    assert pred.grad.sum() == B * T * S * J
    a2, p2 = pkg.prune_joint_inputs(enc, pred, sb[:, :, None] + torch.arange(S), S)
    assert torch.equal(p2[:, 1:4], p[:, 1:4])


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_workspace_size(lib):
    n = _lib.pruned_workspace_bytes(600, 5, 32)
    assert n % 256 == 0
    assert n >= 32 * 600 * 5 * (8 + 4 + 8 + 16)  # {lpb, lpl}, lse, alpha and the two edge terms in float64 per slot
    assert n < 32 * 600 * 5 * 64                 # no function of V or maxU: the interface has neither
    assert _lib.pruned_workspace_bytes(600, 5, 64) > n and _lib.pruned_workspace_bytes(601, 5, 32) > n
    assert _lib.pruned_workspace_bytes(600, 6, 32) > n
    out = ctypes.c_size_t(0)
    for args in ((0, 5, 32), (600, 0, 32), (600, 65, 32), (600, 5, 0), (1 << 20, 64, 32)):
        assert lib.get_rnnt_pruned_workspace_size(*args, ctypes.byref(out)) == INVALID, args
    assert lib.get_rnnt_pruned_workspace_size(600, 5, 32, None) == INVALID
    assert lib.get_rnnt_pruned_workspace_size(600, 64, 32, ctypes.byref(out)) == 0


def test_argument_validation_needs_no_device(lib):
    fake = ctypes.c_void_p(256)  # never dereferenced: rejected before any launch
    o = _lib.make_options(0, 0, 10, 5)

    def call(acts=fake, grads=fake, sb=fake, labels=fake, ll=fake, il=fake, scale=None, V=28, B=4, S=5, topo=0, costs=fake, ws=fake,
             opts=o, lam=0.0):
        return lib.compute_rnnt_loss_pruned(acts, grads, sb, labels, ll, il, scale, V, B, S, topo, costs, ws, opts, lam)

    for name in ("acts", "sb", "labels", "ll", "il", "ws"):  # a NULL required pointer
        assert call(**{name: None}) == INVALID, name
    assert call(grads=None, costs=None) == INVALID       # nothing to compute
    assert call(V=1) == INVALID and call(V=0) == INVALID  # alphabet_size < 2
    assert call(B=0) == INVALID
    assert call(opts=_lib.make_options(0, 28, 10, 5)) == INVALID   # blank outside [0, V)
    assert call(opts=_lib.make_options(0, -1, 10, 5)) == INVALID
    assert call(S=0) == INVALID and call(S=65) == INVALID and call(S=-1) == INVALID
    assert call(topo=2) == INVALID and call(topo=-1) == INVALID
    assert call(opts=_lib.make_options(0, 0, 10, 0)) == INVALID     # maxU outside [1, 8192]
    assert call(opts=_lib.make_options(0, 0, 10, 8193)) == INVALID
    assert call(opts=_lib.make_options(0, 0, 1 << 20, 5), B=32, S=64) == INVALID  # B maxT S >= 2^31
    assert call(opts=_lib.make_options(0, 0, 10, 5, loc=_lib.RNNT_CPU)) == INVALID  # no CPU fallback in the library
    assert call(ws=ctypes.c_void_p(260)) == INVALID      # misaligned workspace
    for lam in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
        assert call(lam=lam) == INVALID, lam


def test_python_argument_errors():
    acts = torch.zeros(2, 4, 3, 5)
    sb = torch.zeros(2, 4, dtype=torch.int32)
    rest = (torch.ones(2, 2, dtype=torch.int32), torch.tensor([4, 4]), torch.tensor([2, 2]))
    for fn in (pkg.rnnt_loss_pruned, pkg.rnnt_loss_pruned_and_grad):
        with pytest.raises(ValueError, match="acts"):
            fn(acts[0], sb, *rest)                                   # a wrong rank
        with pytest.raises(ValueError, match="band width"):
            fn(torch.zeros(2, 4, 65, 5), sb, *rest)                  # acts.shape[2] not in 1 ... 64
        with pytest.raises(ValueError, match="band width"):
            fn(torch.zeros(2, 4, 0, 5), sb, *rest)
        with pytest.raises(ValueError, match="s_begin"):
            fn(acts, sb[:, :3], *rest)                               # s_begin not matching acts
        with pytest.raises(ValueError, match="s_begin"):
            fn(acts, torch.zeros(2, 4, 2, dtype=torch.int32), *rest)
        with pytest.raises(ValueError, match="s_begin"):
            fn(acts, sb[0], *rest)
        with pytest.raises(TypeError, match="float32"):
            fn(acts.double(), sb, *rest)                             # a non-float32 acts
        with pytest.raises(ValueError, match="topology"):
            fn(acts, sb, *rest, topology="bogus")
        for lam in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match="fastemit_lambda"):
                fn(acts, sb, *rest, fastemit_lambda=lam)
        with pytest.raises(ValueError, match="blank_label"):
            fn(acts, sb, *rest, blank_label=5)
    with pytest.raises(ValueError, match="s_range"):
        pkg.prune_ranges(torch.zeros(2, 4, 3), rest[1], rest[2], 0)
    with pytest.raises(ValueError, match="s_range"):
        pkg.prune_joint_inputs(torch.zeros(2, 4, 3), torch.zeros(2, 3, 3), sb, 65)
    assert pruning.MAX_S_RANGE == 64
