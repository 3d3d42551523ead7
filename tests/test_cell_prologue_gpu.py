"""GPU tests of the patch kernels' prologues (csrc/rnnt_kernels.hip cell_tile_kernel, csrc/rnnt_lin.h): the lsm pass fetches a
cell's label before it stages the logits, the gradient pass reads its per-utterance words in one scalar batch and everything a cell
needs from the lattice in one UNCONDITIONAL vector batch with clamped indices -- what it fetched for an edge the cell does not have
is discarded, never used.  The shapes sit on the edges of those clamps; the workspace and the gradient buffer are NaN before every
call, so a value that was used where it should have been discarded shows.

Costs and gradients against the float64 oracle at the bars of include/rnnt.h (costs 1e-4 max(1, |cost|), gradients 1e-4 absolute),
as tests/test_lin_gpu.py applies them, through compute_rnnt_loss_ex and through the _fwd + _bwd split.  No utterance of these may
be handed back to the log-domain kernels (all four flag words stay 0): the fast kernels are what is tested.
tests/tools/emulate_linear.py puts every utterance of them far inside the certificate (-110 bits and below against the -40 bar, no edge near 2^-100)."""
import functools

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib
from oracle import rnnt_oracle as orc
from tests import fastemit_cases as fc
from tests.test_lin_gpu import Call

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTOL, GTOL = 1e-4, 1e-4  # include/rnnt.h


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need a real MI355X"
    pkg.build()


def _inputs(B, T, U, V, seed, il=None, ll=None, blank=0):
    rng = np.random.default_rng(seed)
    acts = rng.normal(size=(B, T, U, V)).astype(np.float32)
    symbols = np.array([v for v in range(V) if v != blank])
    labels = symbols[rng.integers(0, V - 1, size=(B, max(U - 1, 1)))].astype(np.int32)  # (U == 1: one word nobody may read)
    il = np.full(B, T, np.int32) if il is None else np.asarray(il, np.int32)
    ll = np.full(B, U - 1, np.int32) if ll is None else np.asarray(ll, np.int32)
    return acts, labels, il, ll, blank


def _two_tiles():       # two u-tiles (UU = 17), a partial t-tile, and an utterance with T_b = 1 and U_b = 1
    return _inputs(3, 17, 33, 28, seed=1, il=[17, 9, 1], ll=[32, 5, 0])


def _one_cell():        # one cell; U = 1: the label array is empty
    return _inputs(1, 1, 1, 4, seed=2)


def _no_row_nr():       # N = T + U - 1 = 16 = Nr: row n + 1 of the last diagonal does not exist
    return _inputs(2, 12, 5, 28, seed=3)


def _unaligned():       # V % 4 != 0: the AL = false instantiations; blank is the last symbol
    return _inputs(2, 10, 7, 31, seed=4, blank=30)


def _clamped_labels():  # labels outside [0, V): clamp_label
    acts, labels, il, ll, blank = _inputs(2, 9, 20, 28, seed=5)
    labels[0, 3], labels[0, 11], labels[1, 0], labels[1, 18] = -7, 28, 1000, -1
    return acts, labels, il, ll, blank


CASES = {"two_tiles_B3_T17_U33_V28": _two_tiles, "one_cell_B1_T1_U1_V4": _one_cell, "no_row_Nr_B2_T12_U5_V28": _no_row_nr,
         "unaligned_B2_T10_U7_V31_blank30": _unaligned, "clamped_labels_B2_T9_U20_V28": _clamped_labels}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The inputs and the float64 reference of a case, computed once and shared (read-only) by the tests."""
    acts, labels, il, ll, blank = CASES[name]()
    V = acts.shape[-1]
    c_ref, g_ref = orc.rnnt_loss_and_grad(acts, np.clip(labels, 0, V - 1), il, ll, blank=blank)
    return acts, labels, il, ll, blank, c_ref, g_ref


def _call(name):
    acts, labels, il, ll, blank, c_ref, g_ref = _case(name)
    k = Call(acts, labels, il, ll, poison=True)  # NaN workspace, NaN gradient buffer
    B, T, U, V = k.shape
    k.opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, blank, T, U)
    return k


def _compare(c, g, c_ref, g_ref, il, ll):
    assert np.isfinite(c).all() and np.isfinite(g).all()
    dc = (np.abs(c - c_ref) / np.maximum(1.0, np.abs(c_ref))).max()
    dg = np.abs(g - g_ref).max()
    print(f"max cost error {dc:.3e} (bar {CTOL:g}), max gradient error {dg:.3e} (bar {GTOL:g})")
    assert dc <= CTOL and dg <= GTOL
    for b in range(g.shape[0]):  # padded cells: exact zeros
        assert not g[b, int(il[b]):].any() and not g[b, :, int(ll[b]) + 1:].any()


def _on_the_linear_lattice(k):
    f = k.flags()
    assert not f.any(), f  # no flag raised, state word 0: the fast kernels wrote these results


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_call(name):
    acts, labels, il, ll, blank, c_ref, g_ref = _case(name)
    k = _call(name)
    c, g = k.full()
    _compare(c, g, c_ref, g_ref, il, ll)
    _on_the_linear_lattice(k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_then_backward(name):
    acts, labels, il, ll, blank, c_ref, g_ref = _case(name)
    k = _call(name)
    c = k.fwd()
    g = k.bwd()
    _compare(c, g, c_ref, g_ref, il, ll)
    _on_the_linear_lattice(k)
    one = _call(name)
    c1, g1 = one.full()
    assert np.array_equal(c, c1) and np.array_equal(g, g1)  # the split runs the same kernels


def test_visit_all_on_two_tiles():
    """RNNT_VISIT_ALL: no occupancy floor -- every valid cell is live, every chunk is staged."""
    name = "two_tiles_B3_T17_U33_V28"
    acts, labels, il, ll, blank, c_ref, g_ref = _case(name)
    k = _call(name)
    B, T, U, V = k.shape
    st = k.lib.compute_rnnt_loss_flags(k.acts.data_ptr(), k.grads.data_ptr(), k.labels.data_ptr(), k.ll.data_ptr(), k.il.data_ptr(), None,
                                       V, B, k.costs.data_ptr(), k.ws.data_ptr(), k.opts, _lib.RNNT_VISIT_ALL)
    _lib.check(st, "compute_rnnt_loss_flags")
    c, g = k.result()
    _compare(c, g, c_ref, g_ref, il, ll)
    _on_the_linear_lattice(k)


def test_fastemit_on_two_tiles():
    """The FE instantiations of the gradient kernel, lambda = 0.01, against the FastEmit restatement of tests/fastemit_cases.py."""
    name, lam = "two_tiles_B3_T17_U33_V28", 0.01
    acts, labels, il, ll, blank, c_ref, _ = _case(name)
    _, g_ref = fc.loss_and_grad(acts, labels, il, ll, lam)
    k = _call(name)
    B, T, U, V = k.shape
    st = k.lib.compute_rnnt_loss_fastemit(k.acts.data_ptr(), k.grads.data_ptr(), k.labels.data_ptr(), k.ll.data_ptr(), k.il.data_ptr(), None,
                                          V, B, k.costs.data_ptr(), k.ws.data_ptr(), k.opts, 0, lam)
    _lib.check(st, "compute_rnnt_loss_fastemit")
    c, g = k.result()
    _compare(c, g, c_ref, g_ref, il, ll)
    _on_the_linear_lattice(k)
    plain = _call(name).full()[1]
    assert np.abs(g - plain).max() > 1e-4  # lambda did something
