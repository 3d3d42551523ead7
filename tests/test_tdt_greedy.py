"""Batched greedy TDT decoding on the torch route (tdt.TDTGreedyJoint / tdt_greedy_search_batch on CPU tensors): every scenario of
tests/tdt_decode_cases.py against the float64 restatement of include/rnnt_tdt_greedy.h at every step -- ids, frames, lengths,
emitted and all_done exactly, scores and per-token log-probabilities to 1e-12 -- and against tdt.tdt_greedy_decode per utterance.
The inputs are float64 logits whose two best entries per head are more than 1e-6 apart (asserted on the restatement) or exact
ties by construction."""
import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import tdt
from tests import tdt_decode_cases as tc


class CpuJoint:
    """W1 = I, b1 = 0 in float64: with pred_proj = the case's row the torch route sees tanh(row) @ W2 + b2."""

    def __init__(self, case):
        self.W1 = torch.eye(case.J, dtype=torch.float64)
        self.b1 = torch.zeros(case.J, dtype=torch.float64)
        self.W2 = torch.from_numpy(case.W2).double()
        self.b2 = torch.from_numpy(case.b2).double()
        self.blank_label = case.blank


def cpu_logits(case):
    """logits_fn of the restatement: the same float64 formula in numpy (a NaN row gives NaN logits)."""
    W2, b2 = case.W2.astype(np.float64), case.b2.astype(np.float64)

    def fn(b, t, y):
        with np.errstate(invalid="ignore"):
            return np.tanh(case.pred_row(b, t, y).astype(np.float64)) @ W2 + b2

    return fn


class TorchEngine:
    def __init__(self, case, token_times=True):
        self.case = case
        self.jg = tdt.TDTGreedyJoint(CpuJoint(case), case.durations, token_times=token_times)
        assert not self.jg.engine

    def begin(self, N):
        c = self.case
        ms = None if c.max_symbols is None else torch.tensor(c.max_symbols)
        self.jg.begin(torch.from_numpy(c.enc_proj).double(), torch.tensor(c.frames), ms, c.max_per_frame, N)

    def step(self, rows):
        jg = self.jg
        jg.step(pred_proj=torch.from_numpy(rows).double())
        tt = jg.token_times
        return (jg.emitted.numpy(), int(jg.all_done[0]), jg.lengths.numpy(), jg.scores.numpy(), jg.hyps.numpy(),
                jg.frames.numpy() if tt else None, jg.logp.numpy() if tt else None)

    def grow(self, N):
        while self.jg.hyps.shape[1] < N:
            self.jg.grow_hyps()
        assert self.jg.hyps.shape[1] == N, "the scenario's buffer sizes must double"


BAR = (lambda n, max_lse, s: 1e-12, lambda max_lse, lp: 1e-12)
SCENARIOS = tc.scripted_scenarios(0) + [tc.tie_case(1), tc.pause_case([5, 10, 40], 1)]  # (grow_hyps doubles: 5, 10, 20, 40)


def _run(case, **kw):
    return tc.run_tdt(TorchEngine(case, **kw), case, cpu_logits(case), *BAR)


@pytest.mark.parametrize("case", SCENARIOS, ids=[c.name for c in SCENARIOS])
def test_torch_route_matches_the_restatement_at_every_step(case):
    trace, ref, worst, bar, lworst, lbar = _run(case)
    print(tc.describe(case, ref.ev, worst, bar, lworst, lbar))
    assert trace[-1][0].dtype == np.int32 and trace[-1][3].dtype == np.float64
    # without token times: the same ids, lengths and scores, bitwise
    plain = _run(case, token_times=False)[0]
    assert tc.traces_equal([t[:5] for t in trace], plain)


# (tdt_greedy_decode defines nothing for a head without a finite logit: that scenario is held against the restatement alone)
HOST_LOOP = [c for c in SCENARIOS if "nan-row" not in c.name]


@pytest.mark.parametrize("case", HOST_LOOP, ids=[c.name for c in HOST_LOOP])
def test_torch_route_matches_the_host_loop_per_utterance(case):
    _, ref, *_ = _run(case)
    fn = cpu_logits(case)
    for b in range(case.B):
        tokens, frames = tc.host_loop_decode(tdt.tdt_greedy_decode, fn, case, b)
        n = len(ref.y[b])
        budget = None if case.max_symbols is None else max(int(case.max_symbols[b]), 0)
        assert n == len(tokens) or (budget is not None and n == budget < len(tokens)), (b, n, len(tokens), budget)
        assert list(ref.y[b]) == tokens[:n] and list(ref.frames[b]) == frames[:n], b


def test_the_scenarios_reach_what_they_are_for():
    ev = lambda case: _run(case)[1].ev  # noqa: E731
    for cap in (1, 3):
        e = ev(tc.zero_chain_case(0, cap))
        assert e.capped == 4 + 2 + 4 and e.zero_chains == (cap - 1) * e.capped and e.durations_used == {0}  # (T_b clamped to maxT = 4)
    e = ev(tc.blank_zero_case())
    assert e.blank_d0 == 5 + 3 == e.blanks
    e = ev(tc.jump_past_end_case())
    assert e.jumps_from_last == 4 and e.jumps_past_end == 4
    e = ev(tc.pause_case([5, 10, 40]))
    assert e.paused_steps >= 2
    e = ev(tc.tie_case(0))
    assert e.token_ties >= 8 and e.duration_ties >= 8
    e = ev(tc.nan_row_case())
    assert e.no_finite == 2
    used = set()
    for d in tc.DURATION_SETS:
        e = ev(tc.duration_set_case(d))
        assert e.durations_used <= set(d) and (len(d) < 2 or len(e.durations_used) >= 2), d
        assert e.blanks > 0 and e.steps > 3
        used |= e.durations_used
    assert used == {0, 1, 2, 3, 4, 5, 6, 8}


def test_pause_and_resume_equals_the_unpaused_decode():
    small = _run(tc.pause_case([5, 10, 40]))[0]
    large = _run(tc.pause_case([40]))[0]
    for i in (2, 3, 5, 6):  # lengths, scores, frames, logp: bitwise
        assert small[-1][i].tobytes() == large[-1][i].tobytes()
    assert np.array_equal(small[-1][4], large[-1][4])


def test_a_hypothesis_alone_equals_the_same_one_in_the_batch():
    case = tc.duration_set_case([0, 1, 2, 3, 4])
    full = _run(case)[0][-1]
    for b in (0, 4, 6):
        one = tc.scripted_case("alone", 0, case.V, case.durations, 1, case.maxT, [case.frames[b]], [case.max_symbols[b]],
                               case.max_per_frame, case.blank, lambda _b, t, y, b=b: case.script(b, t, y), [128])
        alone = _run(one)[0][-1]
        assert alone[2][0] == full[2][b] and alone[3][0].tobytes() == full[3][b].tobytes()
        assert np.array_equal(alone[4][0], full[4][b]) and np.array_equal(alone[5][0], full[5][b])


def test_arguments():
    case = tc.duration_set_case([0, 1, 2])
    j = CpuJoint(case)
    with pytest.raises(ValueError, match="durations"):
        tdt.TDTGreedyJoint(j, [0, 2, 1])
    narrow = CpuJoint(case)
    narrow.W2, narrow.b2 = narrow.W2[:, :3], narrow.b2[:3]
    with pytest.raises(ValueError, match="V >= 2"):
        tdt.TDTGreedyJoint(narrow, [0, 1])  # one token column left
    j.blank_label = case.V
    with pytest.raises(ValueError, match="blank"):
        tdt.TDTGreedyJoint(j, case.durations)
    j.blank_label = 0
    jg = tdt.TDTGreedyJoint(j, case.durations)
    with pytest.raises(ValueError, match="max_per_frame"):
        jg.begin(torch.zeros(1, 2, case.J, dtype=torch.float64), torch.tensor([2]), None, 0, 4)
    assert "tdt_greedy_search_batch" in tdt.tdt_greedy_decode.__doc__
    assert pkg.TDTGreedyJoint is tdt.TDTGreedyJoint and pkg.tdt_greedy_search_batch is tdt.tdt_greedy_search_batch


def small_tdt_model(seed, V=11, durations=(0, 1, 2, 3, 4), H=64, J=64, scale=3.0):
    """A prediction network and a joint with V + D columns (H = J = 64, one prediction layer), random weights."""
    torch.manual_seed(seed)
    hp = pkg.HParams(vocab_size=V, mel_bins=4, downsample_factor=2, embedding_size=8, encoder_layers=1, encoder_size=H,
                     projection_size=H, time_reduction_index=0, pred_net_layers=1, pred_net_size=H, joint_net_size=J)
    pred = pkg.model.PredictionNetwork(hp).eval()
    joint = pkg.JointLoss(H, J, V + len(durations))
    with torch.no_grad():
        joint.W2.mul_(scale)  # (wider logits: decisions with a margin)
        joint.b2.normal_(0.0, 0.5)
    return pred, joint


@pytest.mark.parametrize("route", ["torch", "engine"])
def test_search_batch_on_the_cpu_matches_the_host_loop(route):
    """tdt_greedy_search_batch on CPU tensors (both prediction routes run torch there) against tdt_greedy_decode driven by the same
    prediction network, utterance by utterance."""
    dur = [0, 1, 2, 3, 4]
    pred, joint = small_tdt_model(3)
    B, T = 5, 12
    enc = torch.randn(B, T, 64, generator=torch.Generator().manual_seed(5))
    frames = torch.tensor([12, 7, 0, 1, 9])
    hyps, lengths, scores, fr, lp = tdt.tdt_greedy_search_batch(pred, joint, enc, frames, dur, max_symbols_per_frame=2, check_every=3,
                                                                prediction_route=route, token_times=True)
    assert tdt.LAST_STEPS % 3 == 0 and hyps.dtype == torch.int32
    total = 0
    for b in range(B):
        def fn(t, y, b=b):
            with torch.no_grad():
                g = pred(torch.tensor([[0] + list(y)]))[:, -1, :]
                lg = joint.logits(enc[b : b + 1, t : t + 1], g[:, None, :])[0, 0, 0]
            for head in (lg[:11], lg[11:]):  # the seed's precondition: every decision has a margin the two routes' roundings cannot flip
                top = torch.topk(head, 2).values
                assert float(top[0] - top[1]) > 1e-4
            return lg
        tokens, tframes = tdt.tdt_greedy_decode(fn, int(frames[b]), dur, 0, 2)
        n = int(lengths[b])
        assert hyps[b, :n].tolist() == tokens and fr[b, :n].tolist() == tframes, b
        assert not hyps[b, n:].any() and (fr[b, n:] == -1).all()
        assert float(lp[b, :n].sum()) >= float(scores[b]) - 1e-5  # (the blanks add to the score alone)
        total += n
    assert total >= 5
    # a symbol budget and a small buffer that has to grow
    h2, l2, _ = tdt.tdt_greedy_search_batch(pred, joint, enc, frames, dur, max_length=torch.tensor([3, 3, 3, 3, 3]),
                                            max_symbols_per_frame=2, check_every=1, prediction_route=route)
    assert l2.tolist() == [min(3, int(n)) for n in lengths] and all(h2[b, : l2[b]].tolist() == hyps[b, : l2[b]].tolist() for b in range(B))
