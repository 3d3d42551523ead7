"""Forced alignment on the modified (one symbol per frame) lattice on the MI355X, through the C ABI and the Python surface, against
the float64 restatement of tests/modified_align_cases.py.

Bars (those of tests/test_align_gpu.py).  Optimality: the engine's path, re-scored in float64 from the restatement's log-softmax,
reaches the restatement's best score minus 1e-4 max(1, |best|), `scores` matches that re-scoring within the same bar and
token_logp is within 1e-4.  Exact frames: only where the restatement is decisive -- planted alignments whose every two-predecessor
decision on the best path has a margin of at least 1e-2, ASSERTED on the restatement alone before the engine is looked at -- and
on the scripted lattices, where every sum is exact.  Against the loss: scores <= -cost + 1e-4 max(1, |cost|) with the cost of
rnnt_loss(..., topology="modified") on the same inputs."""
import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib, alignment
from tests import modified_align_cases as mac

pytestmark = pytest.mark.gpu
MARGIN = 1e-2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    pkg.build()
    return torch.device("cuda:0")


def _engine(dev, acts, labels, il, ll, blank=0):
    f, lp, s = pkg.rnnt_align(torch.tensor(acts, device=dev), torch.tensor(labels, device=dev), torch.tensor(il, device=dev),
                              torch.tensor(ll, device=dev), blank_label=blank, topology="modified")
    torch.cuda.synchronize()
    return f.cpu().numpy(), lp.cpu().numpy(), s.cpu().numpy()


def _costs(dev, acts, labels, il, ll, blank=0):
    with torch.no_grad():
        c = pkg.rnnt_loss(torch.tensor(acts, device=dev), torch.tensor(labels, device=dev), torch.tensor(il, device=dev),
                          torch.tensor(ll, device=dev), blank, topology="modified")
    return c.cpu().numpy().astype(np.float64)


def _check_one(ref, Tb, Lb, frames_row, logp_row, score, cost=None, tag=""):
    """One utterance against its restatement; returns the largest deviation relative to the bar's scale."""
    best = ref["score"]
    scale = max(1.0, abs(best))
    bar = 1e-4 * scale
    score = float(score)
    mac.check_valid_path(frames_row, Tb, Lb)
    rescored = mac.score_path(ref["lpb"], ref["lpl"], frames_row[:Lb])
    assert rescored >= best - bar, (tag, rescored, best)
    assert abs(score - rescored) <= bar, (tag, score, rescored)
    assert (logp_row[Lb:] == 0).all()
    want_lp = np.array([ref["lpl"][f, u] for u, f in enumerate(frames_row[:Lb])])
    np.testing.assert_allclose(logp_row[:Lb], want_lp, rtol=0, atol=1e-4)
    if cost is not None:  # the best path is one of the paths the modified loss sums over
        assert score <= -cost + 1e-4 * max(1.0, abs(cost)), (tag, score, cost)
    dlp = float(np.abs(logp_row[:Lb] - want_lp).max()) if Lb else 0.0
    return max((best - rescored) / scale, abs(score - rescored) / scale), dlp


def _check_optimal(acts, labels, il, ll, blank, out, costs=None, tag=""):
    frames, logp, scores = out
    worst, worst_lp = 0.0, 0.0
    for b in range(acts.shape[0]):
        Tb, Lb = int(il[b]), int(ll[b])
        ref = mac.restate(acts[b], labels[b], Tb, Lb, blank)
        w, dlp = _check_one(ref, Tb, Lb, frames[b], logp[b], scores[b], None if costs is None else costs[b], (tag, b))
        worst, worst_lp = max(worst, w), max(worst_lp, dlp)
    print(f"modified align optimality {tag}: worst deviation / max(1, |best|) {worst:.3e}, worst |d token_logp| {worst_lp:.3e}")


# ---- optimality ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("V", [2, 3, 28, 29, 31, 1024])
def test_optimal_on_every_vocabulary(dev, V, where, scale):
    blank = {"first": 0, "middle": V // 2, "last": V - 1}[where]
    rng = np.random.default_rng(V * 100 + blank * 10 + int(scale))
    acts, labels, il, ll = mac.random_case(rng, 4, 40, 21, V, scale=scale, blank=blank)
    ll[-1] = 0
    out = _engine(dev, acts, labels, il, ll, blank)
    _check_optimal(acts, labels, il, ll, blank, out, _costs(dev, acts, labels, il, ll, blank), tag=f"V{V} blank {blank} x{scale}")


EDGE_L = [62, 63, 64, 65, 66, 127, 128, 129, 130, 191, 192, 193, 255, 256, 257]


def test_optimal_at_lane_and_wave_edges(dev):
    """L around 64, 128, 192 and 256 (a lane's last column, 1 / 2 / 3 / 4 / 6 columns per lane), T = L + 3: once in one ragged
    batch on the widest sweep, once each alone on the sweep of its own width.  One restatement per utterance serves both."""
    rng = np.random.default_rng(64)
    B, V = len(EDGE_L), 5
    ll = np.array(EDGE_L, np.int32)
    il = ll + 3
    T, U = int(il.max()), int(ll.max()) + 1
    acts, labels, _, _ = mac.random_case(rng, B, T, U, V, ragged=False)
    refs = [mac.restate(acts[b], labels[b], int(il[b]), int(ll[b])) for b in range(B)]
    frames, logp, scores = _engine(dev, acts, labels, il, ll)
    costs = _costs(dev, acts, labels, il, ll)
    worst = 0.0
    for b in range(B):
        Tb, Lb = int(il[b]), int(ll[b])
        worst = max(worst, _check_one(refs[b], Tb, Lb, frames[b], logp[b], scores[b], costs[b], ("batch", Lb))[0])
        a1 = np.ascontiguousarray(acts[b:b + 1, :Tb, :Lb + 1])
        f1, lp1, s1 = _engine(dev, a1, np.ascontiguousarray(labels[b:b + 1, :Lb]), il[b:b + 1], ll[b:b + 1])
        worst = max(worst, _check_one(refs[b], Tb, Lb, f1[0], lp1[0], s1[0], costs[b], ("alone", Lb))[0])
        # the same utterance on two sweep widths: the same cells in the same order
        assert f1[0].tobytes() == frames[b, :Lb].tobytes() and lp1[0].tobytes() == logp[b, :Lb].tobytes(), Lb
        assert s1[0].tobytes() == scores[b].tobytes(), Lb
    print(f"modified align optimality lane edges: worst deviation / max(1, |best|) {worst:.3e}")


def test_optimal_beyond_1024_columns(dev):
    """B1 T1110 L1100 V4: the 1024-thread sweep (two columns per thread, the crossing through LDS)."""
    rng = np.random.default_rng(1100)
    acts, labels, il, ll = mac.random_case(rng, 1, 1110, 1101, 4, ragged=False)
    out = _engine(dev, acts, labels, il, ll)
    _check_optimal(acts, labels, il, ll, 0, out, _costs(dev, acts, labels, il, ll), tag="B1 T1110 L1100 V4")


def test_optimal_on_a_long_path(dev):
    rng = np.random.default_rng(600)
    acts, labels, il, ll = mac.random_case(rng, 2, 600, 151, 28)
    out = _engine(dev, acts, labels, il, ll)
    _check_optimal(acts, labels, il, ll, 0, out, _costs(dev, acts, labels, il, ll), tag="B2 T600 L150 V28")


# ---- exact frames -------------------------------------------------------------------------------------------------------
def _assert_decisive(acts, labels, il, ll, blank=0):
    refs = []
    for b in range(acts.shape[0]):
        ref = mac.restate(acts[b], labels[b], int(il[b]), int(ll[b]), blank)
        assert ref["min_margin"] >= MARGIN, (b, ref["min_margin"])
        refs.append(ref)
    return refs


@pytest.mark.parametrize("shape,seed", [((8, 120, 40, 28), 160), ((4, 90, 30, 1024), 120), ((2, 1110, 1101, 4), 7)])
def test_exact_frames_on_planted_alignments(dev, shape, seed):
    """Early and late emitters, gain 20, emission frames drawn without replacement (margins verified on the CPU: the smallest on
    these seeds is above 10)."""
    B, T, U, V = shape
    acts, labels, il, ll, emit = mac.planted_case(np.random.default_rng(seed), B, T, U, V, gain=20.0)
    refs = _assert_decisive(acts, labels, il, ll)
    frames, logp, scores = _engine(dev, acts, labels, il, ll)
    costs = _costs(dev, acts, labels, il, ll)
    for b, ref in enumerate(refs):
        Lb = int(ll[b])
        assert (ref["frames"] == emit[b, :Lb]).all()
        assert (frames[b, :Lb] == ref["frames"]).all() and (frames[b, Lb:] == -1).all(), b
        assert abs(float(scores[b]) - ref["score"]) <= 1e-4 * max(1.0, abs(ref["score"]))
        np.testing.assert_allclose(logp[b, :Lb], ref["logp"], rtol=0, atol=1e-5)
        # strongly peaked posteriors: the best path carries the likelihood
        bar = 1e-4 * max(1.0, abs(costs[b]))
        assert float(scores[b]) <= -costs[b] + bar
        assert abs(float(scores[b]) + costs[b]) <= bar, (b, scores[b], costs[b])


@pytest.mark.parametrize("name", sorted(mac.SCRIPTED))
def test_exact_frames_on_scripted_lattices(dev, name):
    """Decisive through exactness: every cell value and every path sum is exact in float32 / float64, so ties are ties on the
    device too and the tie rule alone picks the path -- the score comes back bit for bit."""
    (acts, labels, il, ll), expect = mac.SCRIPTED[name]()
    ref = mac.restate(acts[0], labels[0], int(il[0]), int(ll[0]), mac.SINK_BLANK)
    assert (ref["frames"] == expect).all()
    frames, logp, scores = _engine(dev, acts, labels, il, ll, mac.SINK_BLANK)
    assert (frames[0] == expect).all(), (frames[0], expect)
    assert float(scores[0]) == np.float32(ref["score"])
    assert (logp[0] == ref["logp"].astype(np.float32)).all()


# ---- structure ----------------------------------------------------------------------------------------------------------
def test_an_utterance_does_not_depend_on_its_batch(dev):
    rng = np.random.default_rng(77)
    T, U, V = 70, 25, 28
    acts, labels, il, ll = mac.random_case(rng, 64, T, U, V, scale=2.0)
    il[5], ll[5] = 61, 19
    alone = _engine(dev, acts[5:6], labels[5:6], il[5:6], ll[5:6])
    of8 = _engine(dev, acts[:8], labels[:8], il[:8], ll[:8])
    sel = list(range(6, 64)) + [5] + list(range(0, 5))  # position 58 of 64
    of64 = _engine(dev, acts[sel], labels[sel], il[sel], ll[sel])
    for k in range(3):
        assert alone[k][0].tobytes() == of8[k][5].tobytes() == of64[k][58].tobytes(), k
    mac.check_valid_path(alone[0][0], 61, 19)


def _slabbed(dev, acts, labels, il, ll, slab, order_seed=None):
    """The slab feed on a workspace of 0xFF bytes, the slabs in shuffled order."""
    B, T, U, V = acts.shape
    al = alignment._Aligner(B, T, U, V, torch.tensor(labels), torch.tensor(il), torch.tensor(ll), 0, dev, "modified")
    al.ws.fill_(0xFF)
    x = torch.tensor(acts, device=dev)
    starts = list(range(0, T, slab))
    if order_seed is not None:
        np.random.default_rng(order_seed).shuffle(starts)
    for t0 in starts:
        al.cells(x[:, t0:t0 + slab].contiguous(), t0)
    return [o.cpu().numpy() for o in al.path()]


@pytest.mark.parametrize("V", [28, 31, 512])
def test_slabs_in_any_order_give_bitwise_the_one_shot_outputs(dev, V):
    rng = np.random.default_rng(V)
    acts, labels, il, ll = mac.random_case(rng, 4, 70, 12, V, scale=3.0)
    whole = _engine(dev, acts, labels, il, ll)
    for slab in (1, 7, 70):
        out = _slabbed(dev, acts, labels, il, ll, slab, order_seed=slab)
        for k in range(3):
            assert out[k].tobytes() == whole[k].tobytes(), (slab, k)
    for b in range(4):
        mac.check_valid_path(whole[0][b], int(il[b]), int(ll[b]))


def test_more_labels_than_frames_and_bad_lengths_are_contained(dev):
    rng = np.random.default_rng(13)
    acts, labels, il, ll = mac.random_case(rng, 7, 30, 10, 28, ragged=False)
    good = _engine(dev, acts, labels, il, ll)
    il2, ll2 = il.copy(), ll.copy()
    il2[1], ll2[2], il2[3], ll2[4] = 0, 10, 31, -1  # out of range
    il2[5], ll2[5] = 4, 9                            # more labels than frames: no path
    frames, logp, scores = _engine(dev, acts, labels, il2, ll2)
    assert np.isnan(scores[1:5]).all() and (frames[1:5] == -1).all() and (logp[1:5] == 0).all()
    assert scores[5] == -np.inf and (frames[5] == -1).all() and (logp[5] == 0).all()
    assert not np.isnan(logp).any()
    for b in (0, 6):
        for k, got in enumerate((frames, logp, scores)):
            assert got[b].tobytes() == good[k][b].tobytes(), (b, k)
    costs = _costs(dev, acts, labels, il2, ll2)
    assert costs[5] == np.inf  # the loss agrees: no path


def test_engine_agrees_with_the_torch_mirror(dev):
    rng = np.random.default_rng(21)
    acts, labels, il, ll, _ = mac.planted_case(rng, 4, 60, 20, 28, gain=20.0)
    _assert_decisive(acts, labels, il, ll)
    eng = _engine(dev, acts, labels, il, ll)
    f, lp, s = pkg.rnnt_align(torch.tensor(acts), torch.tensor(labels), torch.tensor(il), torch.tensor(ll), topology="modified")
    assert (eng[0] == f.numpy()).all()
    np.testing.assert_allclose(eng[2], s.numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(eng[1], lp.numpy(), rtol=0, atol=1e-5)


@pytest.mark.parametrize("V", [32, 128])
def test_fused_route_equals_alignment_of_the_joint_logits(dev, V):
    """align_joint (logits slab by slab) against rnnt_align on joint.cell_logits, both on the modified lattice: bitwise, for any
    slab size.  V = 32: the f32 joint; V = 128: the f16 joint."""
    torch.manual_seed(V)
    B, T, U, H, J = 2, 12, 6, 32, 64
    assert pkg.joint._auto_joint_dtype(J, V) == ("f32" if V == 32 else "f16")
    joint = pkg.JointLoss(H, J, V).to(dev)
    enc, pred = torch.randn(B, T, H, device=dev), torch.randn(B, U, H, device=dev)
    labels = torch.randint(1, V, (B, U - 1), dtype=torch.int32, device=dev)
    il = torch.tensor([12, 7], dtype=torch.int32, device=dev)
    ll = torch.tensor([5, 3], dtype=torch.int32, device=dev)
    with torch.no_grad():
        logits = joint.cell_logits(enc, pred)
        want = [o.cpu().numpy() for o in pkg.rnnt_align(logits, labels, il, ll, blank_label=joint.blank_label, topology="modified")]
        costs = pkg.rnnt_loss(logits, labels, il, ll, joint.blank_label, topology="modified").cpu().numpy()
    for b in range(B):
        mac.check_valid_path(want[0][b], int(il[b]), int(ll[b]))
        assert want[2][b] <= -costs[b] + 1e-4 * max(1.0, abs(costs[b]))
    for slab in (None, 1, 5):
        got = pkg.align_joint(joint, enc, pred, labels, il, ll, slab_frames=slab, topology="modified")
        for k in range(3):
            assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), (slab, k)


@pytest.mark.parametrize("V", [32, 128])
def test_transducer_align_on_the_modified_lattice(dev, V):
    hp = pkg.HParams(vocab_size=V, mel_bins=16, downsample_factor=3, embedding_size=16, encoder_layers=2, encoder_size=64,
                     projection_size=32, time_reduction_index=0, time_reduction_factor=2, pred_net_layers=1, pred_net_size=64,
                     joint_net_size=64)
    torch.manual_seed(0)
    model = pkg.Transducer(hp).to(dev).eval()
    mel, pred_inp, spec_len, lab_len, labels = pkg.synthetic_batch(hp, 2, 24, 5, dev)
    frames, logp, scores = model.align(mel, pred_inp, spec_len, lab_len, labels, topology="modified")
    t_len = pkg.reduced_lengths(spec_len, 2)
    assert frames.shape == (2, 5) and int(t_len.max()) == 12
    for b in range(2):
        mac.check_valid_path(frames[b].cpu().numpy(), int(t_len[b]), int(lab_len[b]))
    assert torch.isfinite(scores).all() and (logp <= 0).all()
    with torch.no_grad():
        enc, pred = model(mel, pred_inp)
        costs = pkg.rnnt_loss(model.joint.cell_logits(enc, pred), labels, t_len, lab_len, model.joint.blank_label,
                              topology="modified")
    assert (scores <= -costs + 1e-4 * costs.abs().clamp(min=1)).all()
    secs = pkg.token_times(frames.cpu(), hp, 16000)
    ok = frames.cpu() >= 0
    assert (secs[ok] >= 0).all()
    for b in range(2):
        s = secs[b][ok[b]]
        assert (s[1:] > s[:-1]).all()  # one token per frame: strictly increasing times


def test_graph_replay_is_the_direct_call(dev):
    """The three launches of compute_rnnt_modified_align captured on one stream and replayed onto a poisoned workspace and
    poisoned outputs."""
    rng = np.random.default_rng(51)
    acts, labels, il, ll = mac.random_case(rng, 3, 20, 9, 28)
    want = _engine(dev, acts, labels, il, ll)
    B, T, U, V = acts.shape
    lib = _lib.load_modalign()
    x = torch.tensor(acts, device=dev)
    lab, tl, tll = (torch.tensor(a, device=dev) for a in (labels, il, ll))
    ws = torch.full((_lib.modified_align_workspace_bytes(T, U, B),), 0xFF, dtype=torch.uint8, device=dev)
    frames = torch.full((B, U - 1), -7, dtype=torch.int32, device=dev)
    logp = torch.full((B, U - 1), float("nan"), device=dev)
    scores = torch.full((B,), float("nan"), device=dev)

    def enqueue():
        o = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, T, U)
        return lib.compute_rnnt_modified_align(x.data_ptr(), lab.data_ptr(), tll.data_ptr(), tl.data_ptr(), V, B, frames.data_ptr(),
                                               logp.data_ptr(), scores.data_ptr(), ws.data_ptr(), o)

    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):  # first use outside the capture
        assert enqueue() == 0
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert enqueue() == 0
    for _ in range(2):
        ws.fill_(0xFF)
        frames.fill_(-7)
        logp.fill_(float("nan"))
        scores.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for got, w in zip((frames, logp, scores), want):
            assert got.cpu().numpy().tobytes() == w.tobytes()
