"""CPU tests of forced alignment on the token-and-duration (TDT) lattice: the float64 restatement of tests/tdt_align_cases.py against
a brute force over all paths, and the torch mirror of rnnt_align_tdt / tdt_align_joint (float32 log-softmaxes, float64 sweep, the
tie rule of include/rnnt_tdt_align.h) against the restatement, against rnnt_loss_tdt, on planted alignments and on the scripted exact
lattices.  Bars: those of tests/test_tdt_align_gpu.py."""
import itertools

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from tests import tdt_align_cases as tac
from tests import tdt_cases as tc

MARGIN = 1e-2
D5 = [0, 1, 2, 3, 4]
BRUTE_SETS = [[0, 1, 2], [1, 2], [0, 2], [1], D5]


def _mirror(acts, labels, il, ll, durations, blank=0, sigma=0.0):
    out = pkg.rnnt_align_tdt(torch.tensor(acts), torch.tensor(labels), torch.tensor(il), torch.tensor(ll), durations,
                             blank_label=blank, sigma=sigma)
    return [o.numpy() for o in out]


# ---- the restatement against the brute force ----------------------------------------------------------------------------
@pytest.mark.parametrize("durations", BRUTE_SETS, ids=[str(d) for d in BRUTE_SETS])
def test_restatement_equals_the_brute_force(durations):
    """Every lattice with T <= 6 and L <= 3, no-path cases included: the recurrence finds the maximum over all paths, its
    back-trace is a path of the lattice and that path has the value."""
    rng = np.random.default_rng(len(durations) * 10 + durations[-1])
    nopath = 0
    for T, L in itertools.product(range(1, 7), range(0, 4)):
        x = rng.normal(size=(T, L + 1, 4 + len(durations))) * 2.0
        labels = rng.integers(1, 4, size=L)
        ref = tac.restate(x, labels, T, L, durations, sigma=0.05)
        brute = tac.brute_force_best(ref["wb"], ref["wl"], durations)
        if brute == -np.inf:
            nopath += 1
            assert ref["score"] == -np.inf and (ref["frames"] == -1).all() and tc.brute_force_cost(x, labels, durations) == np.inf
            continue
        assert abs(ref["score"] - brute) <= 1e-12 * max(1.0, abs(brute)), (T, L)
        tac.check_valid_path(ref["frames"], ref["durs"], T, L, durations)
        assert abs(tac.score_path(ref["wb"], ref["wl"], durations, ref["frames"], ref["durs"]) - brute) <= 1e-12 * max(1.0, abs(brute))
        assert ref["score"] <= -tc.brute_force_cost(x, labels, durations, sigma=0.05) + 1e-12
    assert (nopath > 0) == (durations in ([1, 2], [0, 2], [1]))


# ---- the mirror ---------------------------------------------------------------------------------------------------------
def _check_mirror(acts, labels, il, ll, durations, blank, sigma, out, tag=""):
    frames, durs, logp, scores = out
    worst = 0.0
    for b in range(acts.shape[0]):
        Tb, Lb = int(il[b]), int(ll[b])
        ref = tac.restate(acts[b], labels[b], Tb, Lb, durations, blank, sigma)
        best = ref["score"]
        assert (logp[b, Lb:] == 0).all() and not np.isnan(logp[b]).any()
        if best == -np.inf:
            assert scores[b] == -np.inf and (frames[b] == -1).all() and (durs[b] == -1).all() and (logp[b] == 0).all()
            continue
        bar = 1e-4 * max(1.0, abs(best))
        tac.check_valid_path(frames[b], durs[b], Tb, Lb, durations)
        rescored = tac.score_path(ref["wb"], ref["wl"], durations, frames[b, :Lb], durs[b, :Lb])
        assert rescored >= best - bar, (tag, b, rescored, best)
        assert abs(float(scores[b]) - rescored) <= bar, (tag, b, scores[b], rescored)
        want = np.array([ref["wl"][f, u, list(durations).index(d)] + sigma for u, (f, d) in enumerate(zip(frames[b, :Lb], durs[b, :Lb]))])
        np.testing.assert_allclose(logp[b, :Lb], want, rtol=0, atol=1e-4)
        worst = max(worst, (best - rescored) / max(1.0, abs(best)), abs(float(scores[b]) - rescored) / max(1.0, abs(best)))
    print(f"tdt align mirror {tag}: worst deviation / max(1, |best|) {worst:.3e}")


@pytest.mark.parametrize("sigma", [0.0, 0.05])
@pytest.mark.parametrize("durations,blank", [(D5, 0), ([1, 2], 3), ([0, 2], 6), ([0, 1, 2, 3, 4, 5, 6, 8], 2), ([1, 2, 3, 8], 0)])
def test_mirror_is_optimal_and_below_the_loss(durations, blank, sigma):
    lengths = [(14, 5), (9, 3), (12, 0), (1, 0), (11, 6), (4, 5)]
    acts, labels, il, ll = tc.ragged_case(lengths, 7, len(durations), seed=durations[-1] + blank, scale=2.0, blank=blank)
    out = _mirror(acts, labels, il, ll, durations, blank, sigma)
    _check_mirror(acts, labels, il, ll, durations, blank, sigma, out, tag=f"{durations} sigma {sigma}")
    costs = pkg.rnnt_loss_tdt(torch.tensor(acts), torch.tensor(labels), torch.tensor(il), torch.tensor(ll), durations, blank, sigma).numpy()
    for b in range(len(lengths)):
        if np.isfinite(costs[b]):
            assert out[3][b] <= -costs[b] + 1e-4 * max(1.0, abs(costs[b])), (b, out[3][b], costs[b])
        else:
            assert out[3][b] == -np.inf


PLANTED = [((40, 12, 28), D5), ((64, 63, 5), D5), ((100, 30, 8), D5), ((300, 70, 28), D5), ((24, 7, 7), [0, 1, 2])]


@pytest.mark.parametrize("shape,durations", PLANTED, ids=[str(s) for s, _ in PLANTED])
def test_planted_alignments_are_recovered(shape, durations):
    """Five seeds per shape.  Exact equality is demanded of the mirror only after the restatement ALONE has shown the smallest margin
    on its best path to be at least 1e-2 (measured: above 15 on every seed); the planted path is the best path, and it carries the
    likelihood (seed 0: |score + cost| within 1e-4 max(1, |cost|), measured below 5e-5)."""
    T, L, V = shape
    smallest = np.inf
    for seed in range(5):
        acts, labels, il, ll, pf, pd = tac.planted_case(seed, 1, T, L, V, durations)
        ref = tac.restate(acts[0], labels[0], T, L, durations)
        assert ref["min_margin"] >= MARGIN, (seed, ref["min_margin"])
        smallest = min(smallest, ref["min_margin"])
        assert (ref["frames"] == pf[0]).all() and (ref["durs"] == pd[0]).all(), seed
        if seed == 0:
            cost = -tc.alphas(ref["wb"], ref["wl"], durations)[T, L]
            assert ref["score"] <= -cost and abs(ref["score"] + cost) <= 1e-4 * max(1.0, abs(cost)), (ref["score"], cost)
        if seed < 2:
            frames, durs, logp, scores = _mirror(acts, labels, il, ll, durations)
            assert (frames[0] == pf[0]).all() and (durs[0] == pd[0]).all(), seed
            assert abs(float(scores[0]) - ref["score"]) <= 1e-4 * max(1.0, abs(ref["score"]))
            np.testing.assert_allclose(logp[0], ref["logp"], rtol=0, atol=1e-4)
            ends = pkg.token_end_frames(torch.tensor(frames[0]), torch.tensor(durs[0])).numpy()
            assert (ends == pf[0] + pd[0]).all() and (ends[:-1] <= frames[0][1:]).all()
    print(f"tdt align planted {shape} {durations}: smallest margin on a best path {smallest:.2f}")


@pytest.mark.parametrize("name", sorted(tac.SCRIPTED))
def test_scripted_lattices(name):
    """The restatement on every script: the expected frames and durations, the expected score EXACTLY, equal to the brute force
    EXACTLY (every path sum is exact in float64).  The mirror, whose weights are float32: bit for bit the same wherever the weights
    are float32 numbers; on the script that is exact in float64 alone the raised weight rounds back onto the others and the mirror
    must return the all-tie path."""
    (acts, labels, il, ll), ef, ed, es = tac.SCRIPTED[name]()
    dur = list(tac.SCRIPT_DURATIONS)
    T, L = int(il[0]), int(ll[0])
    ref = tac.restate(acts[0], labels[0], T, L, dur, tac.SCRIPT_BLANK)
    # exactness: every log-probability is its logit, so every weight is a sum of two of the script's dyadic numbers
    lp, ld, _, _, _ = tc.weights(acts[0].astype(np.float64), labels[0], dur, tac.SCRIPT_BLANK)
    assert (lp[..., :2] == acts[0][..., :2]).all() and (ld[..., :3] == acts[0][..., 3:6]).all()
    assert (ref["frames"] == ef).all() and (ref["durs"] == ed).all(), (ref["frames"], ref["durs"])
    assert es is None or ref["score"] == es
    assert ref["score"] == tac.brute_force_best(ref["wb"], ref["wl"], dur)
    assert tac.float32_exact(ref) == (name not in tac.SCRIPTED_F64_ONLY)
    frames, durs, logp, scores = _mirror(acts, labels, il, ll, dur, tac.SCRIPT_BLANK)
    if name in tac.SCRIPTED_F64_ONLY:
        (_, _, _, _), tf, td, ts = tac.SCRIPTED["all_tie"]()
        assert (frames[0] == tf).all() and (durs[0] == td).all() and scores[0] == np.float32(ts)
        return
    assert (frames[0] == ef).all() and (durs[0] == ed).all(), (frames[0], durs[0])
    assert scores[0] == np.float32(ref["score"]) and (logp[0] == ref["logp"].astype(np.float32)).all()


def test_scripted_ulp_moves_the_path():
    """One ulp on one label edge changes the path: both ulp scripts leave the all-tie path for the same other one."""
    (_, _, _, _), tf, td, _ = tac.SCRIPTED["all_tie"]()
    for name in ("ulp", "ulp32"):
        (_, _, _, _), ef, ed, _ = tac.SCRIPTED[name]()
        assert (ef == [0, 2, 3, 5, 6]).all() and (ed == [2, 1, 2, 1, 0]).all() and not (ef == tf).all()


# ---- containment --------------------------------------------------------------------------------------------------------
def test_no_path_bad_lengths_empty_transcripts_and_one_frame():
    durations = [1, 2]
    acts, labels, il, ll = tc.full_case(8, 12, 6, 7, 2, seed=13)
    good = _mirror(acts, labels, il, ll, durations)
    il2, ll2, lab2 = il.copy(), ll.copy(), labels.copy()
    il2[1], ll2[2], il2[3], ll2[4] = 0, 7, 13, -1  # out of range
    il2[5] = 6                                      # L >= T: no path
    lab2[6, 2], lab2[6, 4] = -5, 99                 # clamped to 0 and V - 1
    frames, durs, logp, scores = _mirror(acts, lab2, il2, ll2, durations)
    assert np.isnan(scores[1:5]).all() and (frames[1:5] == -1).all() and (durs[1:5] == -1).all() and (logp[1:5] == 0).all()
    assert scores[5] == -np.inf and (frames[5] == -1).all() and (durs[5] == -1).all() and (logp[5] == 0).all()
    assert not np.isnan(logp).any()
    for b in (0, 7):
        for k, got in enumerate((frames, durs, logp, scores)):
            assert got[b].tobytes() == good[k][b].tobytes(), (b, k)
    clamped = labels.copy()
    clamped[6, 2], clamped[6, 4] = 0, 6
    _check_mirror(acts[6:7], clamped[6:7], il[6:7], ll[6:7], durations, 0, 0.0, [frames[6:7], durs[6:7], logp[6:7], scores[6:7]])
    # L = 0 (blank edges alone), T = 1 (one blank of duration 1), {0, 2} with an odd T, U = 1
    acts, labels, il, ll = tc.ragged_case([(9, 0), (1, 0), (1, 1), (8, 3)], 6, 3, seed=2)
    frames, durs, logp, scores = _mirror(acts, labels, il, ll, [0, 1, 2])
    assert (frames[:2] == -1).all() and (durs[:2] == -1).all() and np.isfinite(scores[:2]).all()
    ref = tac.restate(acts[1], labels[1], 1, 0, [0, 1, 2])
    assert abs(float(scores[1]) - ref["wb"][0, 0, 1]) <= 1e-5
    assert np.isfinite(scores[2]) and frames[2, 0] == 0 and durs[2, 0] == 0  # one frame: the label over d = 0, then the blank
    acts, labels, il, ll = tc.ragged_case([(9, 3), (8, 3)], 6, 2, seed=2)
    frames, durs, logp, scores = _mirror(acts, labels, il, ll, [0, 2])
    assert scores[0] == -np.inf and (frames[0] == -1).all() and np.isfinite(scores[1]) and (durs[1] % 2 == 0).all()
    acts, labels, il, ll = tc.full_case(2, 5, 0, 4, 2, seed=3)
    frames, durs, logp, scores = _mirror(acts, labels, il, ll, [1, 2])
    assert frames.shape == (2, 0) and durs.shape == (2, 0) and logp.shape == (2, 0) and np.isfinite(scores).all()


# ---- the Python surface -------------------------------------------------------------------------------------------------
def test_python_checks():
    acts, labels, il, ll = (torch.tensor(a) for a in tc.full_case(2, 6, 3, 5, 3, seed=1))
    ok = lambda **kw: pkg.rnnt_align_tdt(kw.get("acts", acts), kw.get("labels", labels), kw.get("il", il), kw.get("ll", ll),  # noqa: E731
                                         kw.get("durations", [0, 1, 2]), kw.get("blank", 0), kw.get("sigma", 0.0))
    assert len(ok()) == 4
    for bad in ([0, 2, 1], [2, 3], [0], [0, 1, 9], [], [0, 1.5], "ab", list(range(9))):
        with pytest.raises(ValueError):
            ok(durations=bad)
    for sigma in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ok(sigma=sigma)
    with pytest.raises(TypeError):
        ok(acts=acts.to(torch.float16))
    with pytest.raises(ValueError):
        ok(acts=acts[0])
    with pytest.raises(ValueError):
        ok(labels=labels[:, :2])
    with pytest.raises(ValueError):
        ok(il=il[:1])
    with pytest.raises(ValueError):
        ok(blank=5)  # inside the duration head
    with pytest.raises(ValueError):
        ok(durations=[0, 1, 2, 3, 4, 5, 6])  # seven durations leave V = 1


def test_python_checks_durations_that_leave_too_few_tokens():
    acts, labels, il, ll = (torch.tensor(a) for a in tc.full_case(1, 4, 2, 2, 2, seed=1))  # V + D = 4
    with pytest.raises(ValueError):
        pkg.rnnt_align_tdt(acts, labels, il, ll, [0, 1, 2])  # V = 1


def test_joint_route_on_the_cpu_and_token_times():
    """tdt_align_joint on CPU tensors: the mirror on the joint's logits, slab by slab, equal to the one-shot call; token_times and
    token_end_frames on its outputs."""
    torch.manual_seed(3)
    B, T, U, H, J, R = 2, 9, 5, 8, 16, 11
    joint = pkg.JointLoss(H, J, R)
    enc, pred = torch.randn(B, T, H), torch.randn(B, U, H)
    labels = torch.randint(1, R - 5, (B, U - 1), dtype=torch.int32)
    il, ll = torch.tensor([9, 6], dtype=torch.int32), torch.tensor([4, 2], dtype=torch.int32)
    with torch.no_grad():
        want = pkg.rnnt_align_tdt(joint.cell_logits(enc, pred), labels, il, ll, D5, blank_label=joint.blank_label, sigma=0.05)
    for slab in (None, 1, 4):
        got = pkg.tdt_align_joint(joint, enc, pred, labels, il, ll, D5, slab_frames=slab, sigma=0.05)
        for g, w in zip(got, want):
            assert torch.equal(g, w), slab
    with pytest.raises(ValueError):
        pkg.tdt_align_joint(joint, enc, pred, labels, il, ll, D5, slab_frames=0)
    with pytest.raises(ValueError):
        pkg.tdt_align_joint(joint, enc, pred, labels, il, ll, [0, 1, 2, 3, 4, 5, 6, 7, 8])
    frames, durs = want[0], want[1]
    ends = pkg.token_end_frames(frames, durs)
    assert ((ends == -1) == (frames == -1)).all() and (ends[frames >= 0] == (frames + durs)[frames >= 0]).all()
    assert (frames[1, 2:] == -1).all() and (ends[1, 2:] == -1).all()
    hp = pkg.HParams(vocab_size=R - 5, mel_bins=16, downsample_factor=3, embedding_size=16, encoder_layers=2, encoder_size=64,
                     projection_size=32, time_reduction_index=0, time_reduction_factor=2, pred_net_layers=1, pred_net_size=64,
                     joint_net_size=64)
    secs = pkg.token_times(frames, hp, 16000)
    assert torch.isnan(secs[frames < 0]).all() and (secs[frames >= 0] >= 0).all()
