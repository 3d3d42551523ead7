"""GPU tests of the pruned training mode: the tiny model of tests/test_pruned_training.py on the device.  Every wiring check is
against the composition of the public DEVICE operators -- the operators' own accuracy is pinned by their suites, and a band is
never compared across CPU and device arithmetic (the occupancies differ in their last bits, and so may the band)."""
import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from tests import prune_ranges_cases as pc
from tests.test_pruned_training import HEAD_KEYS, composed, tiny_batch, tiny_hp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def setup():
    torch.manual_seed(1)
    hp = tiny_hp()
    m = pkg.Transducer(hp, loss="pruned").to(DEV)
    return hp, m, tiny_batch(hp, device=DEV)


def test_train_mode_is_the_composition_of_the_device_operators(setup):
    hp, m, batch = setup
    m.train()
    m.zero_grad()
    costs = m.loss(*batch)
    costs.sum().backward()
    got = {k: p.grad.clone() for k, p in m.named_parameters()}
    last = m.pruned.last_simple_costs.clone(), m.pruned.last_pruned_costs.clone(), m.pruned.last_s_begin.clone()
    m.zero_grad()
    simple, pruned, sb = composed(m, batch)
    ref_costs = 0.5 * simple + 1.0 * pruned
    ref_costs.sum().backward()
    assert costs.is_cuda and costs.dtype == torch.float32 and torch.isfinite(costs).all()
    assert torch.equal(costs, ref_costs)
    assert torch.equal(last[0], simple.detach()) and torch.equal(last[1], pruned.detach()) and torch.equal(last[2], sb)
    for k, p in m.named_parameters():
        ref = p.grad
        assert torch.isfinite(got[k]).all(), k
        bar = 1e-4 * max(1.0, float(ref.abs().max()))
        diff = float((got[k] - ref).abs().max())
        print(f"{k}: max |difference| = {diff:.3e}, bar {bar:.3e}")
        assert diff <= bar, k
    for k in HEAD_KEYS:
        assert got[k].abs().max() > 0, k


def test_the_band_is_the_restatement_on_the_first_pass_occupancies(setup):
    hp, m, batch = setup
    mel, pred_inp, spec_len, lab_len, labels = batch
    m.train()
    with torch.no_grad():
        m.loss(*batch)
        enc, pred = m(mel, pred_inp)
        t_len = pkg.reduced_lengths(spec_len, hp.time_reduction_factor)
        p = m.pruned
        _, occ = pkg.rnnt_loss_simple(p.am_head(enc), p.lm_head(pred), labels, t_len, lab_len, m.joint.blank_label,
                                      p.lm_only_scale, p.am_only_scale, p.topology)
    ref = pc.ranges(occ.cpu().numpy(), t_len.cpu().numpy(), lab_len.cpu().numpy(), p.s_range)
    assert np.array_equal(p.last_s_begin.cpu().numpy(), ref)
    pc.check_invariants(ref, t_len.cpu().numpy(), lab_len.cpu().numpy(), p.s_range, occ.shape[2])


def test_eval_mode_is_the_joint_loss(setup):
    hp, m, batch = setup
    mel, pred_inp, spec_len, lab_len, labels = batch
    m.eval()
    with torch.no_grad():
        costs = m.loss(*batch)
        enc, pred = m(mel, pred_inp)
        ref = m.joint(enc, pred, labels, pkg.reduced_lengths(spec_len, hp.time_reduction_factor), lab_len)
    assert torch.isfinite(costs).all() and torch.equal(costs, ref)


def test_one_train_step_logs_the_two_parts():
    torch.manual_seed(5)
    hp = tiny_hp()
    m = pkg.Transducer(hp, loss="pruned").to(DEV)
    before = m.pruned.am_head.weight.detach().clone()
    out = pkg.TrainStep(m, global_batch=3)(*tiny_batch(hp, device=DEV))
    assert set(out) == {"loss", "step_time", "step", "simple_loss", "pruned_loss"}
    assert np.isfinite([out["loss"], out["simple_loss"], out["pruned_loss"]]).all()
    assert out["loss"] == pytest.approx(0.5 * out["simple_loss"] + out["pruned_loss"], rel=1e-5)
    assert not torch.equal(before, m.pruned.am_head.weight.detach())
