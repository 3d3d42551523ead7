"""The beam search with several symbols per frame on CPU tensors: joint.MultiBeamJoint's torch mirror and
decoding.beam_search_batch(symbols_per_frame=E) against the float64 restatement of include/rnnt_beam_multi.h
(tests/multibeam_cases.py), the restatement against a brute-force sum over alignments and against the loss oracle."""
import math

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from oracle import rnnt_oracle as orc
from rnnt_speech_recognition_amd import decoding
from rnnt_speech_recognition_amd import joint as jmod
from tests import decode_scripts as ds
from tests import multibeam_cases as mc
from tests.test_frontend import small_model

SCENARIOS = mc.scenarios()


def _joint_module(sj, blank):
    jl = jmod.JointLoss(1, sj.J, sj.V, blank_label=blank).double()
    W2, b2 = sj.weights()
    with torch.no_grad():
        jl.W1.zero_()
        jl.W2.copy_(torch.tensor(W2, dtype=torch.float64))
        jl.b2.copy_(torch.tensor(b2, dtype=torch.float64))
    return jl


class MirrorMulti:
    def __init__(self, sj, B, K, E, N, maxT, frames, blank):
        self.B, self.maxT, self.frames = B, maxT, frames
        self.mj = jmod.MultiBeamJoint(_joint_module(sj, blank), beam=K, symbols_per_frame=E, max_hyp_len=N)
        assert not self.mj.engine

    def begin(self):
        self.mj.begin(torch.zeros(self.B, self.maxT, 1, dtype=torch.float64), torch.tensor(self.frames))
        assert not self.mj.engine

    def step(self, rows):
        with torch.no_grad():
            p, e = self.mj.step(pred_proj=torch.tensor(rows, dtype=torch.float64))
        return p.numpy(), e.numpy()

    def results(self):
        return tuple(x.numpy() for x in self.mj.results())


def _run(sc):
    sj = sc.joint
    eng = MirrorMulti(sj, sc.B, sc.K, sc.E, sc.max_hyp_len, sc.maxT, sc.frames, sc.blank)
    out = mc.run_multibeam(eng, sj, sc.script, sc.B, sc.K, sc.E, sc.max_hyp_len, sc.frames, sc.maxT, sc.blank, sc.steps,
                           lambda b, t, y: sj.snap(sc.script(b, t, y)), sc.ties_allowed)
    mc.check_expectations(sc, out[1])
    print(mc.describe(sc, out[1], out[2], out[3]))
    return out


def test_the_scenario_list_is_whole():
    assert list(SCENARIOS) == mc.NAMES
    for sc in SCENARIOS.values():
        assert sc.B * 2 * sc.K <= 1024 and 1 <= sc.E <= 8 and sc.V <= (32 if sc.dtype == 0 else 128)
    assert any(sc.K == 1 for sc in SCENARIOS.values()) and {1, 8} <= {sc.E for sc in SCENARIOS.values()}
    assert any(sc.blank == sc.V - 1 for sc in SCENARIOS.values()) and any(0 in sc.frames for sc in SCENARIOS.values())


@pytest.mark.parametrize("name", mc.NAMES)
def test_scripted_scenarios_on_the_torch_mirror(name):
    _run(SCENARIOS[name])


def test_merges_happen_across_rounds_and_open_closed_twins_stay_apart():
    """The scenario's events in detail: a closing merged into an entry of an earlier round of the frame, in round 1 and later; an
    open and a closed hypothesis with one sequence side by side (the restatement keeps them apart, and the mirror agreed at every
    step of the run)."""
    ref = _run(SCENARIOS["merges"])[1]
    assert 0 not in ref.ev.merges_by_round and ref.ev.merges_by_round.get(1, 0) >= 1  # (round 0 finds an empty closed list)
    assert ref.ev.open_closed_pairs >= 6 and ref.ev.overflows >= 6


def test_the_frame_with_an_empty_closed_list_empties_the_beam():
    trace, ref, _, _ = _run(SCENARIOS["nan-rows"])
    hyps, lengths, scores = trace[-1]
    assert ref.open[1] == [] and not lengths[1].any() and (scores[1] == -math.inf).all() and not hyps[1].any()
    assert ref.open[0] and ref.open[2]


# ---- exactness without pruning ---------------------------------------------------------------------
def _exact_fn(sj, script):
    """The logits the mirror forms from the scripted rows, in float64: c tanh of the float32 pred_proj row."""
    return lambda b, t, y: sj.c * np.tanh(sj.pred_rows(script(b, t, y))[0, : sj.V].astype(np.float64))


@pytest.mark.parametrize("T,V,E", mc.EXACT_SHAPES)
def test_without_pruning_every_score_is_the_sum_over_alignments(T, V, E):
    """beam 16 holds every hypothesis of these shapes (asserted on the restatement), so each score must be the exact lattice
    sum.  Tolerance: both sides add at most a few hundred float64 terms of magnitude <= |s|: 1e-13 max(1, |s|) is some forty
    times the rounding of either."""
    sj = ds.ScriptedJoint(64, V, 16.0, 0)
    script = mc.softmax_script(7 + T, V)
    fn = _exact_fn(sj, script)
    N = T * E
    eng = MirrorMulti(sj, 1, 16, E, N, T, [T], 0)
    trace, ref, _, _ = mc.run_multibeam(eng, sj, script, 1, 16, E, N, [T], T, 0, T * (E + 1), fn)
    assert ref.ev.max_candidates <= 16 and ref.ev.max_closed <= 16, "the shape prunes: it cannot show exactness"
    hyps, lengths, scores = trace[-1]
    assert scores.dtype == np.float64
    seen, worst = 0, 0.0
    for k, (y, s) in enumerate(ref.open[0]):
        want = mc.brute_force(fn, 0, T, E, 0, y)
        for got in (s, float(scores[0, k])):
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= 1e-13 * max(1.0, abs(want)), (y, got, want)
        if (T, V, E) == (4, 2, 3) and len(y) <= 3:  # k_t <= E binds nothing: the loss on the standard lattice
            x = np.stack([np.stack([fn(0, t, y[:u]) for u in range(len(y) + 1)]) for t in range(T)])
            cost = orc.utterance_cost_and_grad(x, np.asarray(y, np.int32), blank=0)[0]
            assert abs(-cost - float(scores[0, k])) <= 1e-13 * max(1.0, abs(cost)), (y, cost)
            seen += 1
    assert len(ref.open[0]) >= min(16, T * E) and ((T, V, E) != (4, 2, 3) or seen >= 4)
    print(f"(T, V, E) = {(T, V, E)}: {len(ref.open[0])} hypotheses, lists <= {ref.ev.max_candidates}/{ref.ev.max_closed}, "
          f"worst |score - sum| = {worst:.2e}")


# ---- the search the modified rule cannot do -----------------------------------------------------------
def test_more_labels_than_frames_is_found_with_two_symbols_per_frame_and_not_by_the_modified_search():
    V, T, blank = 9, 3, 0
    target = (4, 2, 7, 1, 5)
    script = mc.path_script(5, V, blank, [[[4, 2], [7, 1], [5]]])
    sj = ds.ScriptedJoint(64, V, 16.0, 0)
    eng = MirrorMulti(sj, 1, 4, 2, T * 2, T, [T], blank)
    ref = mc.run_multibeam(eng, sj, script, 1, 4, 2, T * 2, [T], T, blank, T * 3, lambda b, t, y: script(b, t, y))[1]
    assert ref.open[0][0][0] == target and len(target) > T

    class Modified:  # tests/test_decode_scripts.py's MirrorBeam on this script
        def __init__(self):
            self.bj = jmod.BeamJoint(_joint_module(sj, blank), beam=4)

        def begin(self):
            self.bj.begin(torch.zeros(1, T, 1, dtype=torch.float64), torch.tensor([T]))

        def step(self, rows):
            with torch.no_grad():
                p, e = self.bj.step(pred_proj=torch.tensor(rows, dtype=torch.float64))
            return p.numpy(), e.numpy()

        def results(self):
            return tuple(x.numpy() for x in self.bj.results())

    hyps, lengths, _ = ds.run_beam(Modified(), sj, script, 1, 4, [T], T, blank, T, lambda b, t, y: script(b, t, y), check=False)[0][-1]
    assert int(lengths.max()) <= T < len(target)


# ---- decoding.beam_search_batch ------------------------------------------------------------------------
def _model(seed, blank=0):
    model = small_model(seed).double().eval()
    model.joint.blank_label = blank
    return model


def test_without_the_keyword_the_search_is_the_modified_one_to_the_bit():
    model = _model(3)
    torch.manual_seed(11)
    mel = torch.randn(4, 20, 8, dtype=torch.float64)
    spec_lengths = torch.tensor([20, 13, 0, 7])
    with torch.no_grad():
        enc = model.encoder(mel)
        frames = pkg.reduced_lengths(spec_lengths, model.hp.time_reduction_factor)
        plain = decoding.beam_search_batch(model, enc, frames, beam=3)
        none = decoding.beam_search_batch(model, enc, frames, beam=3, symbols_per_frame=None, max_length=None)
        jb = jmod.BeamJoint(model.joint, 3)  # what the function was before it had the keyword
        old = decoding._beam_search(jb, {}, model.prediction, enc, frames, "torch")
        best = decoding.beam_decode_batch(model, mel, spec_lengths, beam=3, symbols_per_frame=None)
    for a, b, c in zip(plain, none, old):
        assert a.dtype == b.dtype == c.dtype and torch.equal(a, b) and torch.equal(a, c)
    assert plain[0].shape == (4, 3, enc.shape[1])
    assert torch.equal(best[0], plain[0][:, 0]) and torch.equal(best[2], plain[2][:, 0])
    with pytest.raises(ValueError):
        decoding.beam_search_batch(model, enc, frames, beam=3, max_length=5)


@pytest.mark.parametrize("E,K,prediction", [(1, 3, "torch"), (2, 4, "torch"), (3, 2, "engine")])
def test_the_keyword_runs_the_rule_on_a_model(E, K, prediction):
    """beam_search_batch(symbols_per_frame=E) with the model's own prediction network against the restatement fed with the
    model's float64 logits of each hypothesis."""
    blank = 0
    model = _model(2 + E, blank)
    with torch.no_grad():
        model.joint.b2[blank] += 0.4
    torch.manual_seed(100 + E)
    B = 3
    mel = torch.randn(B, 16, 8, dtype=torch.float64)
    spec_lengths = torch.tensor([16, 9, 0])
    with torch.no_grad():
        enc = model.encoder(mel)
        frames = pkg.reduced_lengths(spec_lengths, model.hp.time_reduction_factor)
        ids, lengths, scores = decoding.beam_search_batch(model, enc, frames, beam=K, prediction=prediction, symbols_per_frame=E)
        best = decoding.beam_decode_batch(model, mel, spec_lengths, beam=K, prediction=prediction, symbols_per_frame=E)
        capped = decoding.beam_search_batch(model, enc, frames, beam=K, symbols_per_frame=E, max_length=2)
    T = enc.shape[1]
    assert ids.shape == (B, K, T * E) and ids.dtype == torch.int32 and scores.dtype == torch.float64
    assert capped[0].shape == (B, K, 2) and int(capped[1].max()) <= 2
    assert torch.equal(best[0], ids[:, 0]) and torch.equal(best[1], lengths[:, 0]) and torch.equal(best[2], scores[:, 0])

    def fn(b, t, y):
        with torch.no_grad():  # the stateless prediction network over the prefix, as tests/test_beam_search.py's restate
            g = model.prediction(torch.tensor([(0,) + tuple(y)]))[:, -1:, :]
            return model.joint.logits(enc[b: b + 1, t: t + 1], g)[0, 0, 0].double().numpy()

    ref = mc.MultiRestatement(fn, B, K, E, T * E, frames.tolist(), T, blank)
    for _ in range(T * (E + 1)):
        ref.step()
    for b in range(B):
        for k in range(K):
            n = int(lengths[b, k])
            if k < len(ref.open[b]):
                y, s = ref.open[b][k]
                assert ids[b, k, :n].tolist() == list(y), (b, k)
                assert abs(float(scores[b, k]) - s) <= 1e-9 * max(1.0, abs(s)), (b, k, float(scores[b, k]), s)
            else:
                assert n == 0 and float(scores[b, k]) == -math.inf
            assert not ids[b, k, n:].any()
    assert lengths[2, 0] == 0 and scores[2, 0] == 0.0  # no frames: [((), 0)]


def test_the_keyword_refuses_what_it_cannot_do():
    model = _model(1)
    enc = torch.zeros(1, 4, model.joint.W1.shape[0], dtype=torch.float64)
    frames = torch.tensor([4])
    for kw in (dict(token_times=True), dict(context=object()), dict(lm=object())):
        with pytest.raises(ValueError, match="symbols_per_frame"):
            decoding.beam_search_batch(model, enc, frames, beam=2, symbols_per_frame=2, **kw)
    for E in (0, 9):
        with pytest.raises(ValueError):
            decoding.beam_search_batch(model, enc, frames, beam=2, symbols_per_frame=E)
    with pytest.raises(ValueError):
        decoding.beam_search_batch(model, enc, frames, beam=17, symbols_per_frame=2)
    with pytest.raises(ValueError):
        decoding.beam_search_batch(model, enc, frames, beam=2, symbols_per_frame=2, max_length=0)
