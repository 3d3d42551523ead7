"""GPU tests of compute_rnnt_prune_ranges (include/rnnt_prune_ranges.h, libwarprnnt_pruneranges.so): the device result against the
loop restatement of tests/prune_ranges_cases.py, BIT FOR BIT and with no case left out, at the smallest shapes where the two
kernels can go wrong -- the lane stride's edges in U, the scan's chunk edges in T, every S that changes the window loop -- and
the contract around it: nothing beyond the lengths is read, every element of s_begin is written, and a second call, another
stream and a graph replay give the same bits."""
import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib
from tests import prune_ranges_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S_GRID = (1, 2, 5, 33, 64)
U_GRID = (1, 2, 5, 63, 64, 65, 130, 300)
T_GRID = (1, 2, 3, 63, 64, 65, 129, 200)


def _dev(*arrays):
    return [torch.as_tensor(a, device=DEV) for a in arrays]


def _device(occ, il, ll, S):
    sb = pkg.prune_ranges(*_dev(occ, il, ll), S, ordered=True)
    assert sb.dtype == torch.int32 and sb.is_cuda and tuple(sb.shape) == occ.shape[:2]
    return sb.cpu().numpy()


class RangesCall:
    """The tensors of one raw call of the entry point; s_begin starts as 0x5A bytes."""

    def __init__(self, occ, il, ll, S):
        pkg.build()
        self.lib = _lib.load_pruneranges()
        self.occ, self.il, self.ll = _dev(np.ascontiguousarray(occ, np.float32), il.astype(np.int32), ll.astype(np.int32))
        self.B, self.T, self.U = occ.shape
        self.S = S
        self.sb = torch.empty((self.B, self.T), dtype=torch.int32, device=DEV)
        self.poison()

    def poison(self):
        self.sb.view(torch.uint8).fill_(0x5A)

    def enqueue(self, stream=None):
        opts = _lib.make_options((stream or torch.cuda.current_stream()).cuda_stream, 0, self.T, self.U)
        return self.lib.compute_rnnt_prune_ranges(self.occ.data_ptr(), self.il.data_ptr(), self.ll.data_ptr(), self.B, self.S,
                                                  self.sb.data_ptr(), opts)

    def result(self):
        torch.cuda.synchronize()
        return self.sb.cpu().numpy()


# ---- the grid -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", U_GRID)
@pytest.mark.parametrize("S", S_GRID)
def test_device_is_the_restatement_on_the_grid(S, U):
    for i, T in enumerate(T_GRID):
        occ, il, ll = pc.random_case(7, T, U, S, seed=1000 * S + 10 * U + i)
        assert np.array_equal(_device(occ, il, ll, S), pc.ranges(occ, il, ll, S)), (S, U, T)


def test_the_widest_row():
    occ, il, ll = pc.random_case(1, 2, 8192, 64, seed=1)
    assert np.array_equal(_device(occ, il, ll, 64), pc.ranges(occ, il, ll, 64))


def test_many_frames():
    occ, il, ll = pc.random_case(2, 3000, 8, 3, seed=2)
    il[1] = 2999 - 64
    ref = pc.ranges(occ, il, ll, 3)
    assert np.array_equal(_device(occ, il, ll, 3), ref)
    pc.check_invariants(ref, il, ll, 3, 8)


@pytest.mark.parametrize("maker", [pc.exact_case, pc.peaked_case])
def test_ties_and_peaked_rows(maker):
    """exact_case: ties everywhere, the lowest s0 must win through the lane loop and the butterfly.  peaked_case: the order of
    additions decides, so a device sum in any other order shows here."""
    for seed, (B, T, U, S) in enumerate(((7, 9, 13, 5), (5, 66, 70, 2), (4, 5, 131, 33), (3, 4, 200, 64), (6, 7, 150, 5))):
        occ, il, ll = maker(B, T, U, S, seed)
        assert np.array_equal(_device(occ, il, ll, S), pc.ranges(occ, il, ll, S)), (maker.__name__, B, T, U, S)


@pytest.mark.parametrize("topology", ["standard", "modified"])
def test_on_the_device_occupancies_of_the_simple_loss(topology):
    B, T, U, V, S = 3, 70, 40, 6, 5
    am, lm, labels, il, ll = pc.simple_inputs(B, T, U, V, seed=5)
    t = _dev(am, lm, labels, il, ll)
    _, occ, _, _ = pkg.rnnt_loss_simple_and_grad(*t, topology=topology)
    assert occ.dtype == torch.float32
    sb = pkg.prune_ranges(occ, t[3], t[4], S, ordered=True)
    ref = pc.ranges(occ.cpu().numpy(), il, ll, S)  # the same float32 values, copied to the host
    assert np.array_equal(sb.cpu().numpy(), ref)
    pc.check_invariants(ref, il, ll, S, U)


# ---- the contract -----------------------------------------------------------------------------------------------------------
def test_nothing_beyond_the_lengths_is_read():
    for S, (B, T, U) in ((4, (6, 70, 67)), (64, (5, 9, 130)), (1, (4, 5, 9))):
        occ, il, ll = pc.random_case(B, T, U, S, seed=S)
        ref = pc.ranges(occ, il, ll, S)
        poisoned = occ.copy()
        for b in range(B):
            poisoned[b, il[b]:] = np.nan
            poisoned[b, :, ll[b] + 1:] = np.nan
        assert np.array_equal(_device(poisoned, il, ll, S), ref), S


def test_an_utterance_of_nan_occupancies():
    """What the simple loss hands back for an out-of-range length: its own band satisfies the invariants (raw = 0 everywhere,
    then the rule's ends), and its healthy neighbours equal their results alone."""
    B, T, U, S = 5, 70, 30, 4
    occ, il, ll = pc.random_case(B, T, U, S, seed=9)
    bad = occ.copy()
    bad[0] = np.nan
    bad[4, :, :] = np.nan
    got = _device(bad, il, ll, S)
    assert np.array_equal(got, pc.ranges(bad, il, ll, S))
    pc.check_invariants(got, il, ll, S, U)
    for b in (1, 2, 3):
        alone = _device(occ[b:b + 1], il[b:b + 1], ll[b:b + 1], S)
        assert np.array_equal(got[b:b + 1], alone), b


@pytest.mark.parametrize("what,value", [("T", 0), ("T", 71), ("L", -1), ("L", 30)])
def test_out_of_range_lengths_clamp(what, value):
    B, T, U, S = 3, 70, 30, 4
    occ, il, ll = pc.random_case(B, T, U, S, seed=11)
    il_c, ll_c = il.copy(), ll.copy()
    (il if what == "T" else ll)[1] = value
    (il_c if what == "T" else ll_c)[1] = np.clip(value, 1, T) if what == "T" else np.clip(value, 0, U - 1)
    assert np.array_equal(_device(occ, il, ll, S), pc.ranges(occ, il_c, ll_c, S))


def test_every_element_is_written_and_calls_repeat():
    """s_begin poisoned beforehand is fully overwritten; a second call, a call on a non-default stream and a graph replay of the
    two-launch sequence on a stream of its own equal the direct call bit for bit."""
    B, T, U, S = 6, 131, 70, 5
    occ, il, ll = pc.peaked_case(B, T, U, S, seed=13)
    ref = pc.ranges(occ, il, ll, S)
    k = RangesCall(occ, il, ll, S)
    assert k.enqueue() == 0
    base = k.result()
    assert np.array_equal(base, ref)  # (no 0x5A5A5A5A left: the reference has none)
    k.poison()
    assert k.enqueue() == 0 and np.array_equal(k.result(), base)
    side = torch.cuda.Stream(device=DEV)
    k.poison()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert k.enqueue(side) == 0
    side.synchronize()
    assert np.array_equal(k.result(), base)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert k.enqueue() == 0
    for _ in range(2):
        k.poison()
        graph.replay()
        assert np.array_equal(k.result(), base)


def test_two_pass_fused_returns_the_ordered_band():
    B, T, U, J, V, S = 3, 40, 12, 64, 9, 4
    am, lm, labels, il, ll = pc.simple_inputs(B, T, U, V, seed=17)
    g = torch.Generator().manual_seed(0)
    enc, pred = torch.randn(B, T, J, generator=g).to(DEV), torch.randn(B, U, J, generator=g).to(DEV)
    W2, b2 = (0.1 * torch.randn(J, V, generator=g)).to(DEV), torch.zeros(V, device=DEV)
    t = _dev(am, lm, labels, il, ll)
    _, occ = pkg.rnnt_loss_simple(t[0], t[1], *t[2:])
    simple, pruned, sb = pkg.rnnt_loss_two_pass_fused(t[0], t[1], enc, pred, W2, b2, *t[2:], S, ordered_ranges=True)
    assert np.array_equal(sb.cpu().numpy(), pc.ranges(occ.cpu().numpy(), il, ll, S))
    assert torch.isfinite(simple).all() and torch.isfinite(pruned).all()


def test_device_argument_errors():
    occ, il, ll = _dev(np.zeros((2, 4, 5), np.float32), np.array([4, 4], np.int32), np.array([2, 2], np.int32))
    with pytest.raises(TypeError, match="float32"):
        pkg.prune_ranges(occ.double(), il, ll, 2, ordered=True)
    with pytest.raises(ValueError, match="s_range"):
        pkg.prune_ranges(occ, il, ll, 65, ordered=True)
    sb = pkg.prune_ranges(occ.transpose(1, 2).contiguous().transpose(1, 2), il, ll, 2, ordered=True)  # not contiguous: made so
    assert np.array_equal(sb.cpu().numpy(), pc.ranges(np.zeros((2, 4, 5), np.float32), [4, 4], [2, 2], 2))
