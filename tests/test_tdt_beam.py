"""Batched TDT beam search on the torch route (tdt.TDTBeamJoint / tdt_beam_search_batch on CPU tensors): every scenario of
tests/tdt_beam_cases.py against the float64 restatement of include/rnnt_tdt_beam.h at every step -- ids, lengths, cursors, parents,
emitted, frames and durations exactly, scores within the scenario bar (the route computes them in float64 too: they come out far
inside it) -- beam = 1 against tdt_greedy_search_batch, the argument checks, and tdt_beam_search_batch end to end on a tiny model."""
import math
import re

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import tdt
from tests import decode_scripts as ds
from tests import tdt_beam_cases as bc
from tests.test_tdt_greedy import CpuJoint, cpu_logits, small_tdt_model


class TorchEngine:
    def __init__(self, sc, token_times=True):
        self.case = sc.case
        self.jb = tdt.TDTBeamJoint(CpuJoint(sc.case), sc.case.durations, sc.K, token_times=token_times)
        assert not self.jb.engine

    def begin(self):
        c = self.case
        self.jb.begin(torch.from_numpy(c.enc_proj).double(), torch.tensor(c.frames))

    def step(self, rows):
        parents, emitted = self.jb.step(pred_proj=torch.from_numpy(rows).double())
        return parents.numpy(), emitted.numpy()

    def results(self):
        out = self.jb.results()
        return tuple(x.numpy() for x in out[:3]) + (self.jb.cursors().numpy(),) + tuple(x.numpy() for x in out[3:])


SCENARIOS = bc.scripted_scenarios(0) + bc.scripted_scenarios(1)  # (joint_dtype 1: the logits that survive the binary16 rounding)


def _run(sc, **kw):
    return bc.run_tdt_beam(TorchEngine(sc), sc, cpu_logits(sc.case), **kw)


@pytest.mark.parametrize("sc", SCENARIOS, ids=[s.name for s in SCENARIOS])
def test_torch_route_matches_the_restatement_at_every_step(sc):
    trace, ref, worst, bar = _run(sc)
    print(bc.describe(sc, ref.ev, worst, bar))
    bc.check_expectations(sc, ref.ev)
    assert worst <= 1e-9  # (float64 on both sides)
    # room for the engine: the GPU runs assert the same precondition on the logits entry's f32 logits, up to 16 c 2^-22 away
    assert sc.case.ties_allowed or ref.ev.worst_gap_ratio > 3.0, ref.ev.worst_gap_ratio
    assert trace[-1][0].dtype == np.int32 and trace[-1][2].dtype == np.float64


def test_the_scenarios_cover_what_they_are_for():
    used, levels = set(), set()
    ev = {}
    for sc in SCENARIOS:
        ev[sc.name] = e = bc.dry_run(sc, cpu_logits(sc.case)).ev
        used |= e.durations_used
        levels |= e.tie_levels
    assert used == {0, 1, 2, 3, 4, 5, 6, 8} and levels == {"i", "v", "j"}
    assert {sc.K for sc in SCENARIOS} == {1, 2, 4, 16}
    assert any(e.idle_full > 0 for e in ev.values()) and any(e.past_end > 0 for e in ev.values())
    assert any(e.stay_merges > 0 for e in ev.values()) and any(e.d0_d1_merges > 0 for e in ev.values())
    assert any(e.kept_apart > 0 and e.aligned_later > 0 for e in ev.values())
    e = ev["nan-rows-K4-dt0"]
    assert e.carried == [(1, 0), (3, 4)] and e.dropped >= 1
    # duration jumps save joint rows: fewer active rows than occupied slots
    e = ev["long-jumps-K4-dt0"]
    assert e.active_rows < 4 * e.frames / 2
    # T_b = 0 and T_b = 1 are in every ragged batch
    assert all({0, 1} <= set(sc.case.frames) for sc in SCENARIOS if sc.case.B >= 4)


def test_hash_collision_does_not_merge():
    """Two sequences of equal length, equal rolling hash and equal cursor that differ in their tokens stay two hypotheses: on the
    torch route by construction, and the same scenario runs through the kernels in tests/test_tdt_beam_gpu.py.  The hash constant
    of tdt_beam_kernels.hip is beam_kernels.hip's."""
    sc, want0, want1 = bc.collision_scenario()
    mul = ds.hash_multiplier()
    src = open(ds.BEAM_SOURCE.replace("beam_kernels.hip", "tdt_beam_kernels.hip")).read()
    assert int(re.search(r"kHashMul\s*=\s*(0x[0-9A-Fa-f]+)", src).group(1), 16) == mul
    assert int(re.search(r"kBeamMax\s*=\s*(\d+)", src).group(1)) == 16
    assert ds.rolling_hash(want0, mul) == ds.rolling_hash(want1, mul) and want0 != want1
    trace, ref, worst, bar = bc.run_tdt_beam(TorchEngine(sc, token_times=True), sc, cpu_logits(sc.case), every_step=False)
    hyps, lengths = trace[-1][0], trace[-1][1]
    assert lengths[0].tolist() == [1280, 1280]
    assert hyps[0, 0, :1280].tolist() == list(want0) and hyps[0, 1, :1280].tolist() == list(want1)
    assert ref.ev.merges == 0


@pytest.mark.parametrize("durations", [[0, 1, 2, 3, 4], [1, 2], [0, 2]], ids=str)
def test_beam_1_is_greedy_with_one_symbol_per_frame(durations):
    case = bc.random_scenario(durations, 1, seed=77).case
    joint = CpuJoint(case)
    B, T = case.B, case.maxT
    enc = torch.from_numpy(case.enc_proj).double()
    frames = torch.tensor(case.frames)
    jb = tdt.TDTBeamJoint(joint, durations, 1, token_times=True)
    jg = tdt.TDTGreedyJoint(joint, durations, token_times=True)
    jb.begin(enc, frames)
    jg.begin(enc, frames, None, 1, T)
    yb, yg, tg = [()] * B, [()] * B, [0] * B
    rows = lambda ys, ts: torch.from_numpy(np.stack([case.pred_row(b, ts[b], ys[b]) for b in range(B)])).double()  # noqa: E731
    for t in range(T):
        _, em = jb.step(pred_proj=rows(yb, [t] * B))
        yb = [y + ((int(e),) if e >= 0 else ()) for y, e in zip(yb, em.tolist())]
    while int(jg.all_done[0]) == 0:
        em = jg.step(pred_proj=rows(yg, [min(x, T - 1) for x in tg]))
        yg = [y + ((int(e),) if e >= 0 else ()) for y, e in zip(yg, em.tolist())]
        tg = jg._t.tolist()
    hyps, lengths, scores, fr, du = jb.results()
    assert lengths[:, 0].tolist() == jg.lengths.tolist() and sum(lengths[:, 0].tolist()) >= 5
    for b in range(B):
        n = int(lengths[b, 0])
        assert hyps[b, 0, :n].tolist() == jg.hyps[b, :n].tolist() and fr[b, 0, :n].tolist() == jg.frames[b, :n].tolist(), b
        assert abs(float(scores[b, 0]) - float(jg.scores[b])) <= 1e-9 * max(1.0, abs(float(scores[b, 0])))


def test_arguments():
    case = bc.d0_d1_scenario(2).case
    j = CpuJoint(case)
    for beam in (0, 17, -1):
        with pytest.raises(ValueError, match="beam must be in 1 ... 16"):
            tdt.TDTBeamJoint(j, case.durations, beam)
    with pytest.raises(ValueError, match="durations"):
        tdt.TDTBeamJoint(j, [0, 2, 1])
    j.blank_label = case.V
    with pytest.raises(ValueError, match="blank"):
        tdt.TDTBeamJoint(j, case.durations)
    j.blank_label = 0
    pred, joint = small_tdt_model(3)
    with pytest.raises(ValueError):
        tdt.tdt_beam_search_batch(pred, joint, torch.zeros(1, 2, 64), torch.tensor([2]), [0, 1, 2, 3, 4], prediction_route="nope")
    assert pkg.TDTBeamJoint is tdt.TDTBeamJoint and pkg.tdt_beam_search_batch is tdt.tdt_beam_search_batch
    assert "rnnt_tdt_beam.h" in tdt.TDTBeamJoint.__doc__


@pytest.mark.parametrize("route", ["torch", "engine"])
def test_search_batch_end_to_end_on_a_tiny_model(route):
    """tdt_beam_search_batch on CPU tensors (both prediction routes run torch there): sorted n-best lists, the caller's sequences,
    frames inside the utterance, beam = 1 equal to tdt_greedy_search_batch(max_symbols_per_frame=1)."""
    dur = [0, 1, 2, 3, 4]
    pred, joint = small_tdt_model(3)
    B, T = 5, 12
    enc = torch.randn(B, T, 64, generator=torch.Generator().manual_seed(5))
    frames = torch.tensor([12, 7, 0, 1, 9])
    hyps, lengths, scores, fr, du = tdt.tdt_beam_search_batch(pred, joint, enc, frames, dur, beam=4, prediction_route=route,
                                                              token_times=True, count_active=True)
    assert hyps.shape == (B, 4, T) and hyps.dtype == torch.int32 and lengths.shape == scores.shape == (B, 4)
    assert lengths[2].tolist() == [0, 0, 0, 0] and scores[2].tolist() == [0.0] + [-math.inf] * 3  # T_b = 0: the start beam
    assert (tdt.LAST_ACTIVE_ROWS <= 4 * frames).all() and int(tdt.LAST_ACTIVE_ROWS[0]) >= 1
    for b in range(B):
        s = scores[b].tolist()
        assert s == sorted(s, reverse=True)
        for k in range(4):
            n = int(lengths[b, k])
            assert (fr[b, k, :n] < frames[b]).all() and (fr[b, k, :n] >= 0).all() and (du[b, k, :n] >= 1).all()
            assert (fr[b, k, 1:n] >= fr[b, k, : n - 1] + du[b, k, : n - 1]).all() if n > 1 else True  # one symbol per frame, jumps kept
            assert (fr[b, k, n:] == -1).all() and (du[b, k, n:] == -1).all() and not hyps[b, k, n:].any()
    h1, l1, s1, f1, _ = tdt.tdt_beam_search_batch(pred, joint, enc, frames, dur, beam=1, prediction_route=route, token_times=True)
    hg, lg, sg, fg, _ = tdt.tdt_greedy_search_batch(pred, joint, enc, frames, dur, max_symbols_per_frame=1, prediction_route=route,
                                                    token_times=True)
    assert l1[:, 0].tolist() == lg.tolist() and int(lg.sum()) >= 5
    for b in range(B):
        n = int(lg[b])
        assert h1[b, 0, :n].tolist() == hg[b, :n].tolist() and f1[b, 0, :n].tolist() == fg[b, :n].tolist()
    assert torch.allclose(s1[:, 0].double(), sg.double(), atol=1e-5)
    # the n-best of the wider beam begins at least as well as greedy
    assert (scores[:, 0] >= s1[:, 0] - 1e-6).all()


def test_n_best_scores_stay_below_the_lattice_total():
    """Every n-best score is a sum over SOME paths of that sequence's TDT lattice, so it is at most -rnnt_loss_tdt(sigma = 0) of the
    sequence.  The lattice has no edge that jumps past T and no label edge onto T, which the decoder may take: the case has no
    duration 0, and its last two frames are made blank frames with d = 1 far ahead (their encoder rows saturate the joint's tanh
    onto a sign pattern that the blank column and the d = 1 column of W2 are aligned with, 19 nats), so a hypothesis's paths lie
    in the lattice up to e^-19 of its mass."""
    dur = [1, 2]
    V = 11
    pred, joint = small_tdt_model(11, V=V, durations=dur)
    T, B, K = 10, 3, 4
    enc = torch.randn(B, T, 64, generator=torch.Generator().manual_seed(9))
    frames = [10, 6, 8]
    u = torch.sign(torch.randn(64, generator=torch.Generator().manual_seed(10)))
    with torch.no_grad():
        s = torch.sign(u @ joint.W1)
        for b, n in enumerate(frames):
            enc[b, n - 2 : n] = 50.0 * u
        joint.W2[:, 0] += 0.3 * s
        joint.W2[:, V] += 0.3 * s
    fl = torch.tensor(frames)
    hyps, lengths, scores = tdt.tdt_beam_search_batch(pred, joint, enc, fl, dur, beam=K)
    checked = 0
    for b in range(B):
        for k in range(K):
            if scores[b, k] == -math.inf:
                continue
            n = int(lengths[b, k])
            y = hyps[b, k, :n].tolist()
            with torch.no_grad():
                g = pred(torch.tensor([[0] + y]))  # [1, n + 1, H]
                acts = joint.logits(enc[b : b + 1, : frames[b]], g)
            cost = tdt.rnnt_loss_tdt(acts.double(), torch.tensor([y + [0] * (1 if n == 0 else 0)], dtype=torch.int32)[:, : max(n, 1)],
                                     torch.tensor([frames[b]], dtype=torch.int32), torch.tensor([n], dtype=torch.int32), dur, 0, 0.0)
            assert float(scores[b, k]) <= -float(cost[0]) + 1e-6, (b, k, float(scores[b, k]), -float(cost[0]))
            checked += 1
    assert checked >= 2 * B and int(lengths.sum()) >= 6
