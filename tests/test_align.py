"""Forced alignment on the CPU: the torch mirror of alignment.rnnt_align against the float64 restatement (tests/align_cases.py),
the tie rule on scripted lattices, path validity, a brute-force maximum on tiny lattices, the C ABI's argument checks (no device
needed) and the frame -> time / token -> word helpers.

Bars.  Scores: 1e-4 max(1, |score|), the op's bar for costs in include/rnnt.h (relative, with the floor of 1 that bar has: a
planted lattice's best path has a log-probability of -1e-5, where float32 cell values cannot be 1e-9 accurate).  Paths: identical wherever every two-predecessor decision
on the restatement's best path has a margin of at least 1e-2 -- the mirror's values differ from the restatement's by the float32
rounding of the cell log-probabilities, a few 1e-7 per step, orders of magnitude below that margin."""
import ctypes

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib, alignment, features
from tests import align_cases as ac

MARGIN = 1e-2


def _bar(x):
    return 1e-4 * max(1.0, abs(x))


def _mirror(acts, labels, il, ll, blank=0):
    f, lp, s = pkg.rnnt_align(torch.tensor(acts), torch.tensor(labels), torch.tensor(il), torch.tensor(ll), blank_label=blank)
    return f.numpy(), lp.numpy(), s.numpy()


def _check_against_restatement(acts, labels, il, ll, blank, out, exact_paths="margin"):
    frames, logp, scores = out
    scores = np.asarray(scores, dtype=np.float64)  # (a float32 scalar would pull the comparisons down to float32)
    decisive = 0
    for b in range(acts.shape[0]):
        Tb, Ub = int(il[b]), int(ll[b])
        ref = ac.restate(acts[b], labels[b], Tb, Ub, blank)
        ac.check_valid_path(frames[b], Tb, Ub)
        assert abs(scores[b] - ref["score"]) <= _bar(ref["score"]), (b, scores[b], ref["score"])
        # the returned path, re-scored in float64, IS the returned score
        rescored = ac.score_path(ref["lpb"], ref["lpl"], frames[b, :Ub])
        assert abs(scores[b] - rescored) <= _bar(rescored), (b, scores[b], rescored)
        assert rescored >= ref["score"] - _bar(ref["score"])
        assert (logp[b, Ub:] == 0).all()
        if exact_paths == "always" or ref["min_margin"] >= MARGIN:
            decisive += 1
            assert (frames[b, :Ub] == ref["frames"]).all(), (b, frames[b, :Ub], ref["frames"])
            np.testing.assert_allclose(logp[b, :Ub], ref["logp"], rtol=0, atol=1e-5)
    return decisive


@pytest.mark.parametrize("B,T,U,V,blank,scale", [
    (4, 12, 6, 28, 0, 1.0), (3, 1, 5, 5, 0, 1.0), (3, 9, 1, 7, 0, 1.0), (5, 20, 9, 31, 30, 4.0), (2, 7, 4, 2, 1, 1.0),
    (6, 33, 17, 60, 3, 8.0), (2, 70, 3, 128, 0, 1.0),
])
def test_mirror_agrees_with_the_restatement(B, T, U, V, blank, scale):
    rng = np.random.default_rng(B * 1000 + T * 10 + U)
    acts, labels, il, ll = ac.random_case(rng, B, T, U, V, scale=scale, blank=blank)
    if U > 1:
        ll[-1] = 0  # an utterance without labels: all blanks
    out = _mirror(acts, labels, il, ll, blank)
    _check_against_restatement(acts, labels, il, ll, blank, out)
    if U > 1:
        assert (out[0][-1] == -1).all()


def test_paths_are_identical_where_the_margin_holds():
    """Planted alignments (gain 20): the restatement's best path is decisive everywhere -- asserted, not assumed -- so the mirror
    has to return exactly that path; it is the planted one."""
    rng = np.random.default_rng(5)
    acts, labels, il, ll, emit = ac.planted_case(rng, 6, 40, 11, 28, gain=20.0)
    for b in range(6):
        ref = ac.restate(acts[b], labels[b], int(il[b]), int(ll[b]))
        assert ref["min_margin"] >= MARGIN, (b, ref["min_margin"])
        assert (ref["frames"] == emit[b, : ll[b]]).all()
    out = _mirror(acts, labels, il, ll)
    assert _check_against_restatement(acts, labels, il, ll, 0, out, exact_paths="always") == 6


@pytest.mark.parametrize("name", sorted(ac.SCRIPTED))
def test_tie_rule_on_scripted_lattices(name):
    (acts, labels, il, ll), expect = ac.SCRIPTED[name]()
    ref = ac.restate(acts[0], labels[0], int(il[0]), int(ll[0]), ac.SINK_BLANK)
    assert (ref["frames"] == expect).all(), (ref["frames"], expect)  # the restatement follows the hand-derived path
    frames, logp, scores = _mirror(acts, labels, il, ll, ac.SINK_BLANK)
    assert (frames[0] == expect).all(), (frames[0], expect)
    assert float(scores[0]) == np.float32(ref["score"])  # exact lattice: no rounding anywhere but the final float32
    assert (logp[0] == ref["logp"].astype(np.float32)).all()


def test_scripted_values_are_exact_in_float32():
    """What the scripted lattices rest on: the log-softmax of (x, y, 0) with x, y <= -40 returns x and y exactly."""
    (acts, _, _, _), _ = ac.scripted_ulp()
    lp = torch.log_softmax(torch.tensor(acts), -1).numpy()
    assert (lp[..., :2] == acts[..., :2]).all() and (lp[..., 2] == 0).all()
    assert (ac.log_softmax(acts)[..., :2] == acts[..., :2].astype(np.float64)).all()


@pytest.mark.parametrize("T,U1", [(1, 4), (5, 1), (4, 4), (6, 5), (10, 3), (3, 8)])
def test_score_is_the_maximum_over_all_paths(T, U1):
    rng = np.random.default_rng(T * 31 + U1)
    acts, labels, il, ll = ac.random_case(rng, 1, T, U1, 6, scale=2.0, ragged=False)
    lpb, lpl = ac.cell_logprobs(acts[0], labels[0], T, U1 - 1, 0)
    best = ac.brute_force_best(lpb, lpl)
    assert abs(ac.restate(acts[0], labels[0], T, U1 - 1)["score"] - best) <= 1e-12 * max(1.0, abs(best))
    _, _, scores = _mirror(acts, labels, il, ll)
    assert abs(scores[0] - best) <= _bar(best)


def test_out_of_range_lengths_are_contained():
    rng = np.random.default_rng(11)
    acts, labels, il, ll = ac.random_case(rng, 5, 10, 6, 9, ragged=False)
    good = _mirror(acts, labels, il, ll)
    il2, ll2 = il.copy(), ll.copy()
    il2[1], ll2[2], il2[3], ll2[4] = 0, 6, 11, -1
    frames, logp, scores = _mirror(acts, labels, il2, ll2)
    assert np.isnan(scores[1:]).all() and (frames[1:] == -1).all() and (logp[1:] == 0).all()
    assert scores[0] == good[2][0] and (frames[0] == good[0][0]).all()


def test_align_joint_on_cpu_equals_rnnt_align_on_its_logits():
    torch.manual_seed(3)
    joint = pkg.JointLoss(16, 32, 12)
    enc, pred = torch.randn(3, 14, 16), torch.randn(3, 6, 16)
    labels = torch.randint(1, 12, (3, 5), dtype=torch.int32)
    il, ll = torch.tensor([14, 9, 11]), torch.tensor([5, 2, 0])
    with torch.no_grad():
        want = pkg.rnnt_align(joint.cell_logits(enc, pred), labels, il, ll)
    for slab in (None, 1, 5, 14):
        got = pkg.align_joint(joint, enc, pred, labels, il, ll, slab_frames=slab)
        assert (got[0] == want[0]).all()
        torch.testing.assert_close(got[2], want[2], rtol=1e-5, atol=1e-5)  # (a slab's matmul may round differently on the CPU)
    assert alignment.slab_frames_for(16, 300, 100, 4096) == (256 << 20) // (4 * 16 * 100 * 4096)
    assert alignment.slab_frames_for(1, 10, 5, 28) == 10 and alignment.slab_frames_for(64, 10, 8192, 8192) == 1


def test_transducer_align_on_cpu():
    hp = pkg.HParams(vocab_size=29, mel_bins=8, downsample_factor=3, embedding_size=8, encoder_layers=2, encoder_size=16,
                     projection_size=12, time_reduction_index=0, time_reduction_factor=2, pred_net_layers=1, pred_net_size=16,
                     joint_net_size=16)
    torch.manual_seed(0)
    model = pkg.Transducer(hp).eval()
    mel, pred_inp, spec_len, lab_len, labels = pkg.synthetic_batch(hp, 3, 21, 6, "cpu")
    frames, logp, scores = model.align(mel, pred_inp, spec_len, lab_len, labels)
    t_len = pkg.reduced_lengths(spec_len, 2)
    for b in range(3):
        ac.check_valid_path(frames[b].numpy(), int(t_len[b]), int(lab_len[b]))
    assert torch.isfinite(scores).all() and (logp <= 0).all()
    secs = pkg.token_times(frames, hp, 16000)
    audio_seconds = spec_len.double() * hp.downsample_factor * 0.01
    ok = frames >= 0
    assert (secs[ok] >= 0).all() and (secs[ok] < audio_seconds[:, None].expand_as(secs)[ok]).all()


# ---- the C ABI ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    pkg.build()
    return _lib.load()


def test_workspace_size(lib):
    n = _lib.align_workspace_bytes(600, 150, 32)
    assert n % 256 == 0
    assert n >= 32 * 600 * 150 * 8  # two floats per lattice cell
    for bigger in ((1200, 150, 32), (600, 300, 32), (600, 150, 64)):
        m = _lib.align_workspace_bytes(*bigger)
        assert m % 256 == 0 and m > n, bigger
    assert _lib.align_workspace_bytes(10, 1100, 2) > _lib.align_workspace_bytes(10, 1024, 2)  # the wide sweep's layout
    # the size never depends on the vocabulary: the entry point does not even take it
    assert lib.get_rnnt_align_workspace_size.argtypes[:3] == [ctypes.c_int] * 3 and len(lib.get_rnnt_align_workspace_size.argtypes) == 4
    bad = ctypes.c_size_t(0)
    assert lib.get_rnnt_align_workspace_size(0, 150, 32, ctypes.byref(bad)) == 2
    assert lib.get_rnnt_align_workspace_size(600, 9000, 32, ctypes.byref(bad)) == 2
    assert lib.get_rnnt_align_workspace_size(600, 150, 0, ctypes.byref(bad)) == 2
    assert lib.get_rnnt_align_workspace_size(600, 150, 32, None) == 2
    assert lib.get_rnnt_align_workspace_size(1 << 15, 8192, 8, ctypes.byref(bad)) == 2  # B T U >= 2^31


def test_argument_validation_needs_no_device(lib):
    fake, mis4, mis256 = ctypes.c_void_p(256), ctypes.c_void_p(258), ctypes.c_void_p(260)
    ok = _lib.make_options(0, 0, 10, 5)

    def cells(acts=fake, S=10, t0=0, lab=fake, ll=fake, il=fake, V=28, B=4, ws=fake, o=ok):
        return lib.compute_rnnt_align_cells(acts, S, t0, lab, ll, il, V, B, ws, o)

    def path(fr=fake, lp=fake, sc=fake, ll=fake, il=fake, B=4, ws=fake, o=ok):
        return lib.compute_rnnt_align_path(fr, lp, sc, ll, il, B, ws, o)

    def whole(acts=fake, lab=fake, ll=fake, il=fake, V=28, B=4, fr=fake, lp=fake, sc=fake, ws=fake, o=ok):
        return lib.compute_rnnt_align(acts, lab, ll, il, V, B, fr, lp, sc, ws, o)

    cpu = _lib.make_options(0, 0, 10, 5, loc=_lib.RNNT_CPU)
    big = _lib.make_options(0, 0, 10, 9000)
    blank_oob = _lib.make_options(0, 28, 10, 5)
    for fn, ptrs in ((cells, ("acts", "lab", "ll", "il", "ws")), (path, ("fr", "lp", "sc", "ll", "il", "ws")),
                     (whole, ("acts", "lab", "ll", "il", "fr", "lp", "sc", "ws"))):
        for name in ptrs:
            assert fn(**{name: None}) == 2, (fn.__name__, name)
            assert fn(**{name: mis256 if name == "ws" else mis4}) == 2, (fn.__name__, name)
        assert fn(o=cpu) == 2 and fn(o=big) == 2 and fn(B=0) == 2, fn.__name__
    for fn in (cells, whole):
        assert fn(o=blank_oob) == 2 and fn(V=1) == 2 and fn(V=0) == 2, fn.__name__
    assert cells(S=0) == 2 and cells(t0=-1) == 2 and cells(S=6, t0=5) == 2 and cells(S=11) == 2
    huge = _lib.make_options(0, 0, 1 << 15, 8192)
    assert whole(B=8, o=huge) == 2 and path(B=8, o=huge) == 2 and cells(B=8, S=1, o=huge) == 2
    if not torch.cuda.is_available():  # valid arguments pass validation (and then fail for lack of a device, never with 2)
        assert cells() != 2 and path() != 2 and whole() != 2 and cells(S=5, t0=5) != 2


def test_python_surface_checks_its_arguments():
    acts = torch.zeros(2, 3, 2, 4)
    with pytest.raises(ValueError):
        pkg.rnnt_align(acts, torch.ones(2, 2, dtype=torch.int32), torch.tensor([3, 3]), torch.tensor([1, 1]))
    with pytest.raises(TypeError):
        pkg.rnnt_align(acts.double(), torch.ones(2, 1, dtype=torch.int32), torch.tensor([3, 3]), torch.tensor([1, 1]))
    with pytest.raises(ValueError):
        pkg.rnnt_align(acts, torch.ones(2, 1, dtype=torch.int32), torch.tensor([3, 3]), torch.tensor([1, 1]), blank_label=4)


# ---- frames -> seconds, tokens -> words -------------------------------------------------------------------------------
def test_token_times_with_the_default_front_end():
    hp = pkg.HParams()  # frame_step 10 ms, downsample 3, time reduction 2 -> 60 ms per lattice frame
    assert alignment.frame_seconds(hp, 16000) == pytest.approx(0.06, abs=1e-15)
    t = pkg.token_times(torch.tensor([[0, 1, 10, -1]], dtype=torch.int32), hp, 16000)
    assert t.dtype == torch.float64 and t[0, :3].tolist() == pytest.approx([0.0, 0.06, 0.6], abs=1e-12) and torch.isnan(t[0, 3])
    # the step is a whole number of samples, as the front end rounds it: 11025 Hz x 10 ms = 110.25 -> 110 samples
    assert alignment.frame_seconds(hp, 11025) == pytest.approx(110 * 6 / 11025, abs=1e-15)
    # no time reduction inside the encoder -> no factor
    flat = pkg.HParams(time_reduction_index=8, encoder_layers=8)
    assert alignment.frame_seconds(flat, 16000) == pytest.approx(0.03, abs=1e-15)
    assert alignment.frame_seconds(pkg.HParams(downsample_factor=1, time_reduction_factor=4), 8000) == pytest.approx(0.04, abs=1e-15)


def test_word_times_on_the_character_vocabulary():
    enc = features.CharEncoder()
    ids = enc.encode("hi  there's x")
    frames = [2, 2, 3, 4, 5, 5, 6, 9, 9, 10, 11, 12, 20]
    assert len(ids) == len(frames)
    assert pkg.word_times(ids, frames, enc) == [("hi", 2, 2), ("there's", 5, 11), ("x", 20, 20)]
    # padding (-1 frames) ends the utterance; an empty utterance has no words
    assert pkg.word_times(ids + [5, 6], frames + [-1, -1], enc) == pkg.word_times(ids, frames, enc)
    assert pkg.word_times([], [], enc) == [] and pkg.word_times([1, 1], [0, 3], enc) == []
    assert pkg.word_times(torch.tensor(ids[:2]), torch.tensor(frames[:2]), enc) == [("hi", 2, 2)]


def test_alignment_kernels_use_no_scratch(lib):
    """The compiler's resource record of every alignment kernel in the built library: no private segment, no spilled register."""
    import os
    import re
    import subprocess
    import tempfile

    from tests.test_isa_audit import READELF, _code_objects

    if not os.path.exists(READELF):
        pytest.skip("ROCm LLVM tools absent")
    seen = 0
    with tempfile.TemporaryDirectory() as tmp:
        for co in _code_objects(_lib.LIB_PATH, tmp):
            notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True).stdout
            for rec in notes.split(".name:")[1:]:
                name = rec.split()[0]
                if "align_cells_kernel" not in name and "align_path_kernel" not in name:
                    continue
                seen += 1
                assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", rec).group(1)) == 0, name
                m = re.search(r"\.vgpr_spill_count:\s*(\d+)", rec)
                assert m is None or int(m.group(1)) == 0, name
    assert seen == 14 + 8 + 5  # cell pass: 7 group sizes x {wide, scalar loads}; sweep: 8 one-wave widths + 5 wide ones
