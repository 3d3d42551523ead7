"""Forced alignment on the MI355X, through the C ABI and the Python surface, against the float64 restatement of
tests/align_cases.py.

Bars.  Optimality: the engine's path, re-scored in float64 from the restatement's log-softmax, is at least the restatement's best
score minus 1e-4 |best|, and `scores` matches that re-scoring within the same bar (the op's bar for costs; every optimality input
has |best| far above 1).  Exact frames: only where the restatement is decisive -- every two-predecessor decision on its best path
has a margin of at least 1e-2, ASSERTED on the restatement alone before the engine is looked at; the engine's values carry errors
of a few 1e-7 per step, far below that margin, so it has to follow the same path.  Peaked lattices have best scores near 0, where
the bar is the op's 1e-4 max(1, |.|)."""
import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib, alignment
from tests import align_cases as ac

pytestmark = pytest.mark.gpu
MARGIN = 1e-2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    pkg.build()
    return torch.device("cuda:0")


def _engine(dev, acts, labels, il, ll, blank=0):
    f, lp, s = pkg.rnnt_align(torch.tensor(acts, device=dev), torch.tensor(labels, device=dev), torch.tensor(il, device=dev),
                              torch.tensor(ll, device=dev), blank_label=blank)
    torch.cuda.synchronize()
    return f.cpu().numpy(), lp.cpu().numpy(), s.cpu().numpy()


def _costs(dev, acts, labels, il, ll, blank=0):
    with torch.no_grad():
        c = pkg.rnnt_loss(torch.tensor(acts, device=dev), torch.tensor(labels, device=dev), torch.tensor(il, device=dev),
                          torch.tensor(ll, device=dev), blank)
    return c.cpu().numpy().astype(np.float64)


def _check_optimal(acts, labels, il, ll, blank, out, costs=None, tag=""):
    frames, logp, scores = out
    scores = np.asarray(scores, dtype=np.float64)  # (a float32 scalar would pull the comparisons down to float32)
    worst = 0.0
    for b in range(acts.shape[0]):
        Tb, Ub = int(il[b]), int(ll[b])
        ref = ac.restate(acts[b], labels[b], Tb, Ub, blank)
        best = ref["score"]
        bar = 1e-4 * abs(best)
        ac.check_valid_path(frames[b], Tb, Ub)
        rescored = ac.score_path(ref["lpb"], ref["lpl"], frames[b, :Ub])
        worst = max(worst, (best - rescored) / abs(best), abs(scores[b] - rescored) / abs(best))
        assert rescored >= best - bar, (tag, b, rescored, best)
        assert abs(scores[b] - rescored) <= bar, (tag, b, scores[b], rescored)
        assert (logp[b, Ub:] == 0).all()
        want_lp = np.array([ref["lpl"][f, u] for u, f in enumerate(frames[b, :Ub])])
        np.testing.assert_allclose(logp[b, :Ub], want_lp, rtol=0, atol=1e-4)
        if costs is not None:  # the best path is one of the paths the loss sums over
            assert scores[b] <= -costs[b] + 1e-4 * max(1.0, abs(costs[b])), (tag, b, scores[b], costs[b])
    print(f"align optimality {tag}: worst relative deviation {worst:.3e}")


@pytest.mark.parametrize("scale", [1.0, 4.0, 8.0])
@pytest.mark.parametrize("V", [2, 28, 31, 60, 128, 1024, 4096])
def test_optimal_on_every_vocabulary(dev, V, scale):
    rng = np.random.default_rng(V * 10 + int(scale))
    blank = 30 if V == 31 else 0  # (the reference's character set with the blank last, as tests/golden/blank_last.npz)
    acts, labels, il, ll = ac.random_case(rng, 3, 50, 20, V, scale=scale, blank=blank)
    ll[-1] = 0
    out = _engine(dev, acts, labels, il, ll, blank)
    _check_optimal(acts, labels, il, ll, blank, out, _costs(dev, acts, labels, il, ll, blank), tag=f"V{V} x{scale}")


@pytest.mark.parametrize("scale", [1.0, 4.0, 8.0])
def test_optimal_at_the_headline_size(dev, scale):
    """BASELINE configs[1]: B32 T600 U150 V28."""
    rng = np.random.default_rng(600 + int(scale))
    acts, labels, il, ll = ac.random_case(rng, 32, 600, 150, 28, scale=scale)
    out = _engine(dev, acts, labels, il, ll)
    _check_optimal(acts, labels, il, ll, 0, out, _costs(dev, acts, labels, il, ll), tag=f"B32 T600 U150 V28 x{scale}")


@pytest.mark.parametrize("scale", [1.0, 4.0, 8.0])
def test_optimal_beyond_1024_columns(dev, scale):
    rng = np.random.default_rng(1100 + int(scale))
    acts, labels, il, ll = ac.random_case(rng, 3, 24, 1100, 5, scale=scale)
    ll[1] = 1030
    out = _engine(dev, acts, labels, il, ll)
    _check_optimal(acts, labels, il, ll, 0, out, _costs(dev, acts, labels, il, ll), tag=f"U1100 x{scale}")


def _assert_decisive(acts, labels, il, ll, blank=0):
    refs = []
    for b in range(acts.shape[0]):
        ref = ac.restate(acts[b], labels[b], int(il[b]), int(ll[b]), blank)
        assert ref["min_margin"] >= MARGIN, (b, ref["min_margin"])
        refs.append(ref)
    return refs


@pytest.mark.parametrize("shape", [(8, 120, 40, 28), (4, 90, 30, 1024), (2, 30, 1100, 6)])
def test_exact_frames_on_planted_alignments(dev, shape):
    """Early and late emitters, gain 20 (margins verified on the CPU: the smallest on these seeds is above 1)."""
    B, T, U, V = shape
    rng = np.random.default_rng(T + U)
    acts, labels, il, ll, emit = ac.planted_case(rng, B, T, U, V, gain=20.0)
    refs = _assert_decisive(acts, labels, il, ll)
    frames, logp, scores = _engine(dev, acts, labels, il, ll)
    costs = _costs(dev, acts, labels, il, ll)
    for b, ref in enumerate(refs):
        Ub = int(ll[b])
        assert (ref["frames"] == emit[b, :Ub]).all()
        assert (frames[b, :Ub] == ref["frames"]).all() and (frames[b, Ub:] == -1).all(), b
        assert abs(scores[b] - ref["score"]) <= 1e-4 * max(1.0, abs(ref["score"]))
        np.testing.assert_allclose(logp[b, :Ub], ref["logp"], rtol=0, atol=1e-5)
        # strongly peaked posteriors: the best path carries the likelihood
        assert scores[b] <= -costs[b] + 1e-4 * max(1.0, abs(costs[b]))
        assert abs(scores[b] + costs[b]) <= 1e-4 * max(1.0, abs(costs[b])), (b, scores[b], costs[b])


@pytest.mark.parametrize("name", sorted(ac.SCRIPTED))
def test_exact_frames_on_scripted_lattices(dev, name):
    """Decisive through exactness, not through a margin: every cell value and every path sum of these lattices is exact in
    float32 / float64 (tests/test_align.py::test_scripted_values_are_exact_in_float32), so ties are ties on the device too and
    the tie rule alone picks the path -- the score must come back bit for bit."""
    (acts, labels, il, ll), expect = ac.SCRIPTED[name]()
    ref = ac.restate(acts[0], labels[0], int(il[0]), int(ll[0]), ac.SINK_BLANK)
    assert (ref["frames"] == expect).all()
    frames, logp, scores = _engine(dev, acts, labels, il, ll, ac.SINK_BLANK)
    assert (frames[0] == expect).all(), (frames[0], expect)
    assert float(scores[0]) == np.float32(ref["score"])
    assert (logp[0] == ref["logp"].astype(np.float32)).all()


def test_an_utterance_does_not_depend_on_its_batch(dev):
    rng = np.random.default_rng(77)
    T, U, V = 70, 25, 28
    acts, labels, il, ll = ac.random_case(rng, 64, T, U, V, scale=2.0)
    il[5], ll[5] = 61, 19
    alone = _engine(dev, acts[5:6], labels[5:6], il[5:6], ll[5:6])
    perm = [0, 1, 2, 3, 4, 5, 6, 7]
    of8 = _engine(dev, acts[perm], labels[perm], il[perm], ll[perm])
    sel = list(range(6, 64)) + [5] + list(range(0, 5))  # position 58 of 64
    of64 = _engine(dev, acts[sel], labels[sel], il[sel], ll[sel])
    for k in range(3):
        assert alone[k][0].tobytes() == of8[k][5].tobytes() == of64[k][58].tobytes(), k


def _slabbed(dev, acts, labels, il, ll, slab, poison):
    B, T, U, V = acts.shape
    al = alignment._Aligner(B, T, U, V, torch.tensor(labels), torch.tensor(il), torch.tensor(ll), 0, dev)
    al.ws.fill_(poison)
    x = torch.tensor(acts, device=dev)
    for t0 in (range(0, T, slab) if slab else [0]):
        al.cells(x[:, t0:t0 + (slab or T)].contiguous(), t0)
    torch.cuda.synchronize()
    planes = al.ws.cpu().numpy().copy()
    out = [o.cpu().numpy() for o in al.path()]
    return planes, out


@pytest.mark.parametrize("V", [28, 31, 512])
def test_slabs_give_bitwise_the_same_planes_and_outputs(dev, V):
    rng = np.random.default_rng(V)
    acts, labels, il, ll = ac.random_case(rng, 4, 70, 12, V, scale=3.0)
    planes0, out0 = _slabbed(dev, acts, labels, il, ll, None, 0)
    whole = _engine(dev, acts, labels, il, ll)
    for k in range(3):
        assert out0[k].tobytes() == whole[k].tobytes()
    for slab in (1, 7, 64):
        planes, out = _slabbed(dev, acts, labels, il, ll, slab, 0)
        assert planes.tobytes() == planes0.tobytes(), slab
        for k in range(3):
            assert out[k].tobytes() == out0[k].tobytes(), (slab, k)
    # a NaN-poisoned workspace changes nothing: cells outside an utterance's lattice are never read
    _, outp = _slabbed(dev, acts, labels, il, ll, 7, 0xFF)
    for k in range(3):
        assert outp[k].tobytes() == out0[k].tobytes(), k


def test_out_of_range_lengths_are_contained(dev):
    rng = np.random.default_rng(13)
    acts, labels, il, ll = ac.random_case(rng, 6, 30, 9, 28, ragged=False)
    good = _engine(dev, acts, labels, il, ll)
    il2, ll2 = il.copy(), ll.copy()
    il2[1], ll2[2], il2[3], ll2[4] = 0, 9, 31, -1
    frames, logp, scores = _engine(dev, acts, labels, il2, ll2)
    assert np.isnan(scores[1:5]).all() and (frames[1:5] == -1).all() and (logp[1:5] == 0).all()
    for b in (0, 5):
        for k, got in enumerate((frames, logp, scores)):
            assert got[b].tobytes() == good[k][b].tobytes(), (b, k)


def test_engine_agrees_with_the_torch_mirror(dev):
    rng = np.random.default_rng(21)
    acts, labels, il, ll, _ = ac.planted_case(rng, 4, 60, 20, 28, gain=20.0)
    eng = _engine(dev, acts, labels, il, ll)
    f, lp, s = pkg.rnnt_align(torch.tensor(acts), torch.tensor(labels), torch.tensor(il), torch.tensor(ll))
    assert (eng[0] == f.numpy()).all()
    np.testing.assert_allclose(eng[2], s.numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(eng[1], lp.numpy(), rtol=0, atol=1e-5)


@pytest.mark.parametrize("V,J", [(28, 64), (4096, 128)])
def test_fused_route_equals_alignment_of_the_joint_logits(dev, V, J):
    """align_joint (logits slab by slab, never [B, T, U, V]) against rnnt_align on the logits joint_logits returns: bitwise.  The
    slab route's peak memory stays under its budget: one slab of logits (slab_bytes) beside the alignment workspace and the
    logits kernels' own workspace for a slab."""
    torch.manual_seed(V)
    B, T, U, H = 4, 64, 24, 32
    joint = pkg.JointLoss(H, J, V).to(dev)
    enc, pred = torch.randn(B, T, H, device=dev), torch.randn(B, U, H, device=dev)
    labels = torch.randint(1, V, (B, U - 1), dtype=torch.int32, device=dev)
    il = torch.tensor([64, 40, 57, 33], dtype=torch.int32, device=dev)
    ll = torch.tensor([23, 11, 0, 17], dtype=torch.int32, device=dev)
    with torch.no_grad():
        logits = pkg.joint_logits(enc, pred, joint.W1, joint.b1, joint.W2, joint.b2)
        want = [o.cpu().numpy() for o in pkg.rnnt_align(logits, labels, il, ll)]
    full_bytes = logits.numel() * 4
    del logits
    budget = full_bytes // 6
    S = alignment.slab_frames_for(B, T, U, V, budget)
    assert 1 <= S < T // 4
    for slab, slab_bytes in ((None, budget), (1, alignment.SLAB_BYTES), (7, alignment.SLAB_BYTES)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        got = pkg.align_joint(joint, enc, pred, labels, il, ll, slab_frames=slab, slab_bytes=slab_bytes)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        for k in range(3):
            assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), (slab, k)
        if slab is None:
            Jp, Vp = pkg.joint.padded_joint_shape(J, V, pkg.joint._auto_joint_dtype(J, V))
            allowed = budget + _lib.align_workspace_bytes(T, U, B) + _lib.joint_net_workspace_bytes(S, U, B, H, Jp, Vp) + (4 << 20)
            print(f"align_joint V{V}: peak {peak} bytes, allowed {allowed}, full logits {full_bytes}")
            assert peak <= allowed, (peak, allowed)
            if V >= 1024:
                assert peak < full_bytes // 2


def test_transducer_align_end_to_end(dev):
    hp = pkg.HParams(vocab_size=29, mel_bins=16, downsample_factor=3, embedding_size=16, encoder_layers=2, encoder_size=64,
                     projection_size=32, time_reduction_index=0, time_reduction_factor=2, pred_net_layers=1, pred_net_size=64,
                     joint_net_size=64)
    torch.manual_seed(0)
    model = pkg.Transducer(hp).to(dev).eval()
    mel, pred_inp, spec_len, lab_len, labels = pkg.synthetic_batch(hp, 4, 60, 9, dev)
    frames, logp, scores = model.align(mel, pred_inp, spec_len, lab_len, labels)
    t_len = pkg.reduced_lengths(spec_len, 2)
    for b in range(4):
        ac.check_valid_path(frames[b].cpu().numpy(), int(t_len[b]), int(lab_len[b]))
    assert torch.isfinite(scores).all() and (logp <= 0).all()
    costs = model.loss(mel, pred_inp, spec_len, lab_len, labels)
    assert (scores <= -costs + 1e-4 * costs.abs().clamp(min=1)).all()
    secs = pkg.token_times(frames.cpu(), hp, 16000)
    audio_seconds = spec_len.cpu().double() * hp.downsample_factor * 0.01
    ok = frames.cpu() >= 0
    assert (secs[ok] >= 0).all() and (secs[ok] < audio_seconds[:, None].expand_as(secs)[ok]).all()
