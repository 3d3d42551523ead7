"""Forced alignment on the token-and-duration (TDT) lattice on the MI355X, through the C ABI (include/rnnt_tdt_align.h) and the Python
surface (rnnt_align_tdt, tdt_align_joint), against the float64 restatement of tests/tdt_align_cases.py.

Bars (those of tests/test_modified_align_gpu.py).  Optimality: the engine's (frames, durations), re-scored in float64 from the
restatement's weights, reach the restatement's best score minus 1e-4 max(1, |best|), `scores` matches that re-scoring within the
same bar and token_logp is within 1e-4.  Exact frames and durations: only where the restatement is decisive -- planted alignments
whose every decision on the best path has a margin of at least 1e-2, ASSERTED on the restatement alone before the engine is looked
at -- and on the scripted lattices whose weights are float32 numbers, where every sum is exact.  Against the loss:
scores <= -cost + 1e-4 max(1, |cost|) with the cost of rnnt_loss_tdt on the same inputs."""
import ctypes

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib, tdt
from tests import tdt_align_cases as tac
from tests import tdt_cases as tc

pytestmark = pytest.mark.gpu
MARGIN = 1e-2
D5 = [0, 1, 2, 3, 4]
D8 = [0, 1, 2, 3, 4, 5, 6, 8]
DURATION_SETS = [D5, [1, 2], [0, 1], [1], [0, 2], D8, [1, 2, 3, 8]]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    pkg.build()
    return torch.device("cuda:0")


def _np(out):
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _engine(dev, acts, labels, il, ll, durations, blank=0, sigma=0.0):
    x = acts if isinstance(acts, torch.Tensor) else torch.tensor(acts, device=dev)
    return _np(pkg.rnnt_align_tdt(x, torch.tensor(labels, device=dev), torch.tensor(il, device=dev), torch.tensor(ll, device=dev),
                                  durations, blank_label=blank, sigma=sigma))


def _costs(dev, acts, labels, il, ll, durations, blank=0, sigma=0.0):
    with torch.no_grad():
        c = pkg.rnnt_loss_tdt(torch.tensor(acts, device=dev), torch.tensor(labels, device=dev), torch.tensor(il, device=dev),
                              torch.tensor(ll, device=dev), durations, blank, sigma)
    return c.cpu().numpy().astype(np.float64)


def _check_one(ref, Tb, Lb, durations, out_b, cost=None, tag=""):
    """One utterance against its restatement; returns the largest deviations (relative to the bar's scale; token_logp absolute)."""
    frames, durs, logp, score = out_b
    best, score = ref["score"], float(score)
    assert not np.isnan(logp).any() and (logp[Lb:] == 0).all(), tag
    if best == -np.inf:  # no path: data, not an error
        assert score == -np.inf and (frames == -1).all() and (durs == -1).all() and (logp == 0).all(), (tag, score, frames)
        if cost is not None:
            assert cost == np.inf, (tag, cost)
        return 0.0, 0.0
    scale = max(1.0, abs(best))
    bar = 1e-4 * scale
    tac.check_valid_path(frames, durs, Tb, Lb, durations)
    rescored = tac.score_path(ref["wb"], ref["wl"], durations, frames[:Lb], durs[:Lb])
    assert rescored >= best - bar, (tag, rescored, best)
    assert abs(score - rescored) <= bar, (tag, score, rescored)
    lp_ref = ref["wl"] + ref.get("sigma", 0.0)  # lp + ld without sigma
    want_lp = np.array([lp_ref[f, u, list(durations).index(d)] for u, (f, d) in enumerate(zip(frames[:Lb], durs[:Lb]))])
    np.testing.assert_allclose(logp[:Lb], want_lp, rtol=0, atol=1e-4)
    if cost is not None:  # the best path is one of the paths the loss sums over
        assert score <= -cost + 1e-4 * max(1.0, abs(cost)), (tag, score, cost)
    dlp = float(np.abs(logp[:Lb] - want_lp).max()) if Lb else 0.0
    return max((best - rescored) / scale, abs(score - rescored) / scale), dlp


def _refs(acts, labels, il, ll, durations, blank=0, sigma=0.0):
    refs = []
    for b in range(acts.shape[0]):
        ref = tac.restate(acts[b], labels[b], int(il[b]), int(ll[b]), durations, blank, sigma)
        ref["sigma"] = sigma
        refs.append(ref)
    return refs


def _check_optimal(refs, il, ll, durations, out, costs=None, tag=""):
    worst, worst_lp = 0.0, 0.0
    for b, ref in enumerate(refs):
        w, dlp = _check_one(ref, int(il[b]), int(ll[b]), durations, [o[b] for o in out], None if costs is None else costs[b], (tag, b))
        worst, worst_lp = max(worst, w), max(worst_lp, dlp)
    print(f"tdt align optimality {tag}: worst deviation / max(1, |best|) {worst:.3e}, worst |d token_logp| {worst_lp:.3e}")


def _same_bits(a, b, tag=""):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (tag, k)


# ---- optimality ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("V,D", [(4, 2), (4, 3), (3, 5), (4, 5), (5, 8), (1030, 5)])
def test_optimal_on_every_row_layout(dev, V, D, where, scale):
    """V + D in {6, 7, 8, 9, 13} and V = 1030 with D = 5; the blank first, in the middle and last; sigma 0 and 0.05; N(0,1) and
    4 N(0,1).  V + D = 8 takes the 16-byte loads: the same tensor at an address off by one float must give the same bits."""
    durations = {2: [1, 2], 3: [0, 1, 2], 5: D5, 8: D8}[D]
    blank = {"first": 0, "middle": V // 2, "last": V - 1}[where]
    acts, labels, il, ll = tc.ragged_case([(12, 5), (9, 3), (11, 0)], V, D, seed=V * 100 + D * 10 + blank + int(scale), scale=scale,
                                          blank=blank)
    for sigma in (0.0, 0.05):
        out = _engine(dev, acts, labels, il, ll, durations, blank, sigma)
        costs = _costs(dev, acts, labels, il, ll, durations, blank, sigma)
        _check_optimal(_refs(acts, labels, il, ll, durations, blank, sigma), il, ll, durations, out, costs,
                       tag=f"V{V} D{D} blank {blank} x{scale} sigma {sigma}")
        if (V + D) % 4 == 0:
            buf = torch.empty(acts.size + 1, device=dev)
            view = buf[1:].view(acts.shape)
            view.copy_(torch.tensor(acts))
            assert view.data_ptr() % 16 == 4 and view.is_contiguous()
            _same_bits(_engine(dev, view, labels, il, ll, durations, blank, sigma), out, "the scalar load route")


@pytest.mark.parametrize("R", [8, 36])
def test_both_load_routes_give_the_same_bits(dev, R):
    """Rows of 8 and 36 floats (one and several chunks per lane group), whole and in slabs: the aligned tensor takes the 16-byte
    loads, the view one float further on the scalar loads."""
    V = R - 5
    acts, labels, il, ll = tc.ragged_case([(20, 7), (13, 9)], V, 5, seed=R, scale=3.0)
    want = _engine(dev, acts, labels, il, ll, D5, sigma=0.05)
    buf = torch.empty(acts.size + 1, device=dev)
    view = buf[1:].view(acts.shape)
    view.copy_(torch.tensor(acts))
    _same_bits(_engine(dev, view, labels, il, ll, D5, sigma=0.05), want)
    _check_optimal(_refs(acts, labels, il, ll, D5, 0, 0.05), il, ll, D5, want, tag=f"load routes R{R}")


EDGE_L = [62, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257]


def test_optimal_at_lane_and_wave_edges(dev):
    """L around 64, 128 and 256 (a wavefront's last column, the sweep's 128-, 256- and 512-thread instantiations) in one ragged
    batch, T = 6."""
    lengths = [(6, L) for L in EDGE_L]
    acts, labels, il, ll = tc.ragged_case(lengths, 4, 5, seed=64)
    out = _engine(dev, acts, labels, il, ll, D5)
    _check_optimal(_refs(acts, labels, il, ll, D5), il, ll, D5, out, _costs(dev, acts, labels, il, ll, D5), tag="lane edges")
    # one of them alone, on the sweep of its own width: the same cells in the same order
    b = EDGE_L.index(65)
    alone = _engine(dev, np.ascontiguousarray(acts[b:b + 1, :, :66]), np.ascontiguousarray(labels[b:b + 1, :65]), il[b:b + 1],
                    ll[b:b + 1], D5)
    _same_bits([alone[0][0], alone[1][0], alone[2][0], alone[3][0]], [out[0][b, :65], out[1][b, :65], out[2][b, :65], out[3][b]])


def test_optimal_at_1024_columns(dev):
    """maxU = 1024 with L = 1022 and 1023, T = 4: the 1024-thread sweep and its 80 KB ring."""
    acts, labels, il, ll = tc.ragged_case([(4, 1022), (4, 1023)], 4, 5, seed=1024)
    out = _engine(dev, acts, labels, il, ll, D5)
    _check_optimal(_refs(acts, labels, il, ll, D5), il, ll, D5, out, _costs(dev, acts, labels, il, ll, D5), tag="B2 T4 L1022/1023")


@pytest.mark.parametrize("durations", DURATION_SETS, ids=[str(d) for d in DURATION_SETS])
def test_frame_edges(dev, durations):
    """T_b in {1, 2, dmax, dmax+1, dmax+2, 2 dmax+3} x L_b in {0, 1, 5} in ONE batch: the terminal rule t + d == T, the wrap of the
    ring, and utterances without a path beside feasible ones."""
    dmax = durations[-1]
    lengths = [(T, L) for T in sorted({1, 2, dmax, dmax + 1, dmax + 2, 2 * dmax + 3}) for L in (0, 1, 5)]
    acts, labels, il, ll = tc.ragged_case(lengths, 6, len(durations), seed=20 + dmax)
    refs = _refs(acts, labels, il, ll, durations)
    feasible = np.array([r["score"] > -np.inf for r in refs])
    if durations in ([1, 2], [1], [0, 2]):
        assert not feasible.all()
    assert feasible.any()
    out = _engine(dev, acts, labels, il, ll, durations)
    _check_optimal(refs, il, ll, durations, out, _costs(dev, acts, labels, il, ll, durations), tag=f"frame edges {durations}")


def test_optimal_on_a_long_path(dev):
    acts, labels, il, ll = tc.ragged_case([(600, 20), (571, 17)], 8, 5, seed=600, scale=8.0)
    out = _engine(dev, acts, labels, il, ll, D5)
    _check_optimal(_refs(acts, labels, il, ll, D5), il, ll, D5, out, _costs(dev, acts, labels, il, ll, D5), tag="B2 T600 L20 V8 x8")


# ---- exact frames and durations -----------------------------------------------------------------------------------------
def _assert_decisive(acts, labels, il, ll, durations):
    refs = _refs(acts, labels, il, ll, durations)
    for b, ref in enumerate(refs):
        assert ref["min_margin"] >= MARGIN, (b, ref["min_margin"])
    return refs


PLANTED = [((40, 12, 28), D5), ((64, 63, 5), D5), ((100, 30, 8), D5), ((24, 7, 7), [0, 1, 2])]


@pytest.mark.parametrize("shape,durations", PLANTED, ids=[str(s) for s, _ in PLANTED])
def test_exact_paths_on_planted_alignments(dev, shape, durations):
    """Gain 20 on the token and the duration of every cell of a planted random walk (margins verified on the CPU: above 15)."""
    T, L, V = shape
    acts, labels, il, ll, pf, pd = tac.planted_case(T + L, 2, T, L, V, durations)
    refs = _assert_decisive(acts, labels, il, ll, durations)
    frames, durs, logp, scores = _engine(dev, acts, labels, il, ll, durations)
    costs = _costs(dev, acts, labels, il, ll, durations)
    for b, ref in enumerate(refs):
        assert (ref["frames"] == pf[b]).all() and (ref["durs"] == pd[b]).all()
        assert (frames[b] == ref["frames"]).all() and (durs[b] == ref["durs"]).all(), b
        assert abs(float(scores[b]) - ref["score"]) <= 1e-4 * max(1.0, abs(ref["score"]))
        np.testing.assert_allclose(logp[b], ref["logp"], rtol=0, atol=1e-4)
        # strongly peaked posteriors: the best path carries the likelihood
        bar = 1e-4 * max(1.0, abs(costs[b]))
        assert float(scores[b]) <= -costs[b] + bar
        assert abs(float(scores[b]) + costs[b]) <= bar, (b, scores[b], costs[b])
        ends = pkg.token_end_frames(torch.tensor(frames[b]), torch.tensor(durs[b])).numpy()
        assert (ends == pf[b] + pd[b]).all() and (ends[:-1] <= frames[b][1:]).all()


@pytest.mark.parametrize("name", sorted(tac.SCRIPTED))
def test_exact_paths_on_scripted_lattices(dev, name):
    """Decisive through exactness: where every weight is a float32 number, every path sum is exact in float64, ties are ties on the
    device too, the tie rule alone picks the path and the score comes back bit for bit.  The script that is exact in float64 alone
    (its raised weight rounds back onto the others in float32) is held to the optimality bars instead."""
    (acts, labels, il, ll), ef, ed, es = tac.SCRIPTED[name]()
    dur = list(tac.SCRIPT_DURATIONS)
    (ref,) = _refs(acts, labels, il, ll, dur, tac.SCRIPT_BLANK)
    assert (ref["frames"] == ef).all() and (ref["durs"] == ed).all() and (es is None or ref["score"] == es)
    out = _engine(dev, acts, labels, il, ll, dur, tac.SCRIPT_BLANK)
    assert tac.float32_exact(ref) == (name not in tac.SCRIPTED_F64_ONLY)
    if name in tac.SCRIPTED_F64_ONLY:
        _check_optimal([ref], il, ll, dur, out, tag=f"scripted {name}")
        return
    frames, durs, logp, scores = out
    assert (frames[0] == ef).all() and (durs[0] == ed).all(), (frames[0], durs[0])
    assert float(scores[0]) == np.float32(ref["score"])
    assert (logp[0] == ref["logp"].astype(np.float32)).all()


# ---- structure ----------------------------------------------------------------------------------------------------------
def test_an_utterance_does_not_depend_on_its_batch(dev):
    lengths = [(int(t), int(l)) for t, l in zip(np.random.default_rng(7).integers(20, 41, 24), np.random.default_rng(8).integers(0, 15, 24))]
    lengths[5] = (37, 11)
    acts, labels, il, ll = tc.ragged_case(lengths, 23, 5, seed=77, scale=2.0)
    T5, U5 = 37, 12
    alone = _engine(dev, np.ascontiguousarray(acts[5:6]), labels[5:6], il[5:6], ll[5:6], D5, sigma=0.05)
    of8 = _engine(dev, acts[:8], labels[:8], il[:8], ll[:8], D5, sigma=0.05)
    sel = list(range(6, 24)) + [5] + list(range(0, 5))  # position 18 of 24
    of24 = _engine(dev, acts[sel], labels[sel], il[sel], ll[sel], D5, sigma=0.05)
    for k in range(4):
        assert alone[k][0].tobytes() == of8[k][5].tobytes() == of24[k][18].tobytes(), k
    # ... nor on maxT and maxU: the same utterance cut out of the padding
    cut = _engine(dev, np.ascontiguousarray(acts[5:6, :T5, :U5]), np.ascontiguousarray(labels[5:6, :U5 - 1]), il[5:6], ll[5:6], D5,
                  sigma=0.05)
    _same_bits([cut[0][0], cut[1][0], cut[2][0], cut[3][0]], [alone[0][0, :U5 - 1], alone[1][0, :U5 - 1], alone[2][0, :U5 - 1], alone[3][0]])
    tac.check_valid_path(alone[0][0], alone[1][0], 37, 11, D5)


def _aligner(dev, acts, labels, il, ll, durations, sigma=0.0, blank=0):
    B, T, U, R = acts.shape
    t = lambda a: torch.tensor(a, device=dev)  # noqa: E731
    return tdt._TDTAligner(B, T, U, R - len(durations), t(labels), t(il), t(ll), tuple(durations), blank, sigma, dev)


def _slabbed(dev, acts, labels, il, ll, durations, slab, order_seed, sigma=0.0, offset=False):
    """The slab feed on a workspace of 0xFF bytes, the slabs in shuffled order (offset: every slab at an address off by one float)."""
    al = _aligner(dev, acts, labels, il, ll, durations, sigma)
    al.ws.fill_(0xFF)
    x = torch.tensor(acts, device=dev)
    starts = list(range(0, acts.shape[1], slab))
    np.random.default_rng(order_seed).shuffle(starts)
    for t0 in starts:
        part = x[:, t0:t0 + slab].contiguous()
        if offset:
            buf = torch.empty(part.numel() + 1, device=dev)
            buf[1:].view(part.shape).copy_(part)
            part = buf[1:].view(part.shape)
        al.cells(part, t0)
    return _np(al.path())


@pytest.mark.parametrize("V", [23, 26, 507])
def test_slabs_in_any_order_give_bitwise_the_one_shot_outputs(dev, V):
    """V + D = 28 and 512 (16-byte loads) and 31 (scalar loads, a padded last chunk): slabs of 1, 7 and all frames, shuffled, on a
    poisoned workspace; once more with every slab at an address off by one float (the scalar route throughout)."""
    acts, labels, il, ll = tc.ragged_case([(70, 11), (55, 8), (64, 0), (70, 3)], V, 5, seed=V, scale=3.0)
    whole = _engine(dev, acts, labels, il, ll, D5, sigma=0.05)
    for slab in (1, 7, 70):
        _same_bits(_slabbed(dev, acts, labels, il, ll, D5, slab, slab, 0.05), whole, slab)
    _same_bits(_slabbed(dev, acts, labels, il, ll, D5, 7, 3, 0.05, offset=True), whole, "offset slabs")
    for b in range(4):
        tac.check_valid_path(whole[0][b], whole[1][b], int(il[b]), int(ll[b]), D5)


def test_two_calls_and_a_side_stream_give_the_same_bits(dev):
    acts, labels, il, ll = tc.ragged_case([(30, 9), (25, 4)], 23, 5, seed=5, scale=2.0)
    first = _engine(dev, acts, labels, il, ll, D5)
    _same_bits(_engine(dev, acts, labels, il, ll, D5), first, "second call")
    side = torch.cuda.Stream(device=dev)
    x = torch.tensor(acts, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out = pkg.rnnt_align_tdt(x, torch.tensor(labels, device=dev), torch.tensor(il, device=dev), torch.tensor(ll, device=dev), D5)
    side.synchronize()
    _same_bits(_np(out), first, "side stream")


def test_no_path_bad_lengths_and_bad_labels_are_contained(dev):
    durations = [1, 2]
    acts, labels, il, ll = tc.full_case(8, 12, 6, 7, 2, seed=13)
    good = _engine(dev, acts, labels, il, ll, durations)
    il2, ll2, lab2 = il.copy(), ll.copy(), labels.copy()
    il2[1], ll2[2], il2[3], ll2[4] = 0, 7, 13, -1  # out of range
    il2[5] = 6                                      # [1, 2] with L >= T: no path
    lab2[6, 2], lab2[6, 4] = -5, 99                 # labels out of range: clamped to 0 and V - 1
    frames, durs, logp, scores = _engine(dev, acts, lab2, il2, ll2, durations)
    assert np.isnan(scores[1:5]).all() and (frames[1:5] == -1).all() and (durs[1:5] == -1).all() and (logp[1:5] == 0).all()
    assert scores[5] == -np.inf and (frames[5] == -1).all() and (durs[5] == -1).all() and (logp[5] == 0).all()
    assert not np.isnan(logp).any()
    for b in (0, 7):
        _same_bits([frames[b], durs[b], logp[b], scores[b]], [g[b] for g in good], b)
    clamped = labels.copy()
    clamped[6, 2], clamped[6, 4] = 0, 6
    (ref,) = _refs(acts[6:7], clamped[6:7], il[6:7], ll[6:7], durations)
    _check_one(ref, 12, 6, durations, [frames[6], durs[6], logp[6], scores[6]], tag="clamped labels")
    costs = _costs(dev, acts, labels, il2, ll2, durations)
    assert costs[5] == np.inf  # the loss agrees: no path
    # durations {0, 2} with an odd T
    acts, labels, il, ll = tc.ragged_case([(9, 3), (8, 3)], 6, 2, seed=2)
    frames, durs, logp, scores = _engine(dev, acts, labels, il, ll, [0, 2])
    assert scores[0] == -np.inf and (frames[0] == -1).all() and (durs[0] == -1).all() and (logp[0] == 0).all()
    assert np.isfinite(scores[1]) and (durs[1] % 2 == 0).all()


def test_engine_agrees_with_the_torch_mirror(dev):
    acts, labels, il, ll, _, _ = tac.planted_case(21, 3, 50, 15, 23, D5)
    _assert_decisive(acts, labels, il, ll, D5)
    eng = _engine(dev, acts, labels, il, ll, D5, sigma=0.05)
    cpu = pkg.rnnt_align_tdt(torch.tensor(acts), torch.tensor(labels), torch.tensor(il), torch.tensor(ll), D5, sigma=0.05)
    assert (eng[0] == cpu[0].numpy()).all() and (eng[1] == cpu[1].numpy()).all()
    np.testing.assert_allclose(eng[3], cpu[3].numpy(), rtol=0, atol=1e-4 * max(1.0, float(np.abs(eng[3]).max())))
    np.testing.assert_allclose(eng[2], cpu[2].numpy(), rtol=0, atol=1e-5)


@pytest.mark.parametrize("R", [33, 1029])
def test_joint_route_equals_alignment_of_the_joint_logits(dev, R):
    """tdt_align_joint (logits slab by slab) against rnnt_align_tdt on joint.cell_logits: bitwise, for any slab size."""
    torch.manual_seed(R)
    B, T, U, H, J = 2, 12, 6, 32, 64
    joint = pkg.JointLoss(H, J, R).to(dev)
    V = R - 5
    enc, pred = torch.randn(B, T, H, device=dev), torch.randn(B, U, H, device=dev)
    labels = torch.randint(1, V, (B, U - 1), dtype=torch.int32, device=dev)
    il = torch.tensor([12, 7], dtype=torch.int32, device=dev)
    ll = torch.tensor([5, 3], dtype=torch.int32, device=dev)
    with torch.no_grad():
        logits = joint.cell_logits(enc, pred)
        want = _np(pkg.rnnt_align_tdt(logits, labels, il, ll, D5, blank_label=joint.blank_label, sigma=0.05))
        costs = pkg.rnnt_loss_tdt(logits, labels, il, ll, D5, joint.blank_label, 0.05).cpu().numpy()
    for b in range(B):
        tac.check_valid_path(want[0][b], want[1][b], int(il[b]), int(ll[b]), D5)
        assert want[3][b] <= -costs[b] + 1e-4 * max(1.0, abs(costs[b]))
    for slab in (None, 1, 5):
        _same_bits(_np(pkg.tdt_align_joint(joint, enc, pred, labels, il, ll, D5, slab_frames=slab, sigma=0.05)), want, slab)


def test_graph_replay_is_the_direct_call(dev):
    """The two launches of compute_rnnt_tdt_align captured on one stream and replayed onto a poisoned workspace and poisoned
    outputs."""
    acts, labels, il, ll = tc.ragged_case([(20, 8), (17, 5), (20, 0)], 23, 5, seed=51)
    want = _engine(dev, acts, labels, il, ll, D5, sigma=0.05)
    B, T, U, R = acts.shape
    lib = _lib.load_tdtalign()
    x = torch.tensor(acts, device=dev)
    lab, tl, tll = (torch.tensor(a, device=dev) for a in (labels, il, ll))
    ws = torch.full((_lib.tdt_align_workspace_bytes(T, U, B, 5),), 0xFF, dtype=torch.uint8, device=dev)
    frames = torch.full((B, U - 1), -7, dtype=torch.int32, device=dev)
    durs = torch.full((B, U - 1), -7, dtype=torch.int32, device=dev)
    logp = torch.full((B, U - 1), float("nan"), device=dev)
    scores = torch.full((B,), float("nan"), device=dev)
    d = (ctypes.c_int * 5)(*D5)

    def enqueue():
        o = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, T, U)
        return lib.compute_rnnt_tdt_align(x.data_ptr(), lab.data_ptr(), tll.data_ptr(), tl.data_ptr(), R - 5, d, 5, 0.05, B,
                                          frames.data_ptr(), durs.data_ptr(), logp.data_ptr(), scores.data_ptr(), ws.data_ptr(), o)

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
        durs.fill_(-7)
        logp.fill_(float("nan"))
        scores.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _same_bits([frames.cpu().numpy(), durs.cpu().numpy(), logp.cpu().numpy(), scores.cpu().numpy()], want)
