"""CPU tests of forced alignment on the modified (one symbol per frame) lattice: they pin the float64 restatement of
tests/modified_align_cases.py against brute force, the torch mirror of alignment.py against the restatement, and check what needs
no device -- the `topology` option, the header, the symbols and the exports of libwarprnnt_modalign.so, and the argument
validation of its entry points."""
import ctypes

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib
from tests import align_cases as ac
from tests import modified_align_cases as mac

INVALID = 2  # RNNT_STATUS_INVALID_VALUE


@pytest.fixture(scope="module")
def lib():
    pkg.build()
    return _lib.load_modalign()


def _mirror(acts, labels, il, ll, blank=0, **kw):
    f, lp, s = pkg.rnnt_align(torch.tensor(acts), torch.tensor(labels), torch.tensor(il), torch.tensor(ll), blank_label=blank,
                              topology="modified", **kw)
    return f.numpy(), lp.numpy(), s.numpy()


# ---- the restatement ----------------------------------------------------------------------------------------------------
def test_restatement_matches_brute_force():
    """300 random lattices, T <= 7, L <= T, V = 4: the recurrence's score is the maximum over all C(T, L) paths, and its
    back-trace is a path with that score."""
    rng = np.random.default_rng(0)
    for _ in range(300):
        T = int(rng.integers(1, 8))
        L = int(rng.integers(0, T + 1))
        acts, labels, _, _ = mac.random_case(rng, 1, T, L + 1, 4, ragged=False)
        ref = mac.restate(acts[0], labels[0], T, L)
        assert abs(ref["score"] - mac.brute_force_best(ref["lpb"], ref["lpl"])) <= 1e-12, (T, L)
        assert abs(mac.score_path(ref["lpb"], ref["lpl"], ref["frames"]) - ref["score"]) <= 1e-12, (T, L)
        mac.check_valid_path(ref["frames"], T, L)


def test_planted_frames_are_drawn_without_replacement():
    rng = np.random.default_rng(5)
    acts, labels, il, ll, emit = mac.planted_case(rng, 6, 30, 13, 8, gain=20.0)
    for b in range(6):
        mac.check_valid_path(emit[b], int(il[b]), int(ll[b]))
        ref = mac.restate(acts[b], labels[b], int(il[b]), int(ll[b]))
        assert ref["min_margin"] >= 1e-2 and (ref["frames"] == emit[b, : ll[b]]).all()


# ---- the torch mirror against the restatement ---------------------------------------------------------------------------
SCRIPTED_FRAMES = {"all_tie": [0, 1, 2, 3, 4], "ulp": [0, 1, 5, 6, 7], "late": [4, 5, 6, 7, 8], "early": [0, 1, 2, 3, 4]}


@pytest.mark.parametrize("name", sorted(mac.SCRIPTED))
def test_mirror_on_scripted_lattices(name):
    """T = 9, L = 5, dyadic values: every sum is exact, so the tie rule alone decides and the score comes back bit for bit."""
    (acts, labels, il, ll), expect = mac.SCRIPTED[name]()
    assert list(expect) == SCRIPTED_FRAMES[name]
    ref = mac.restate(acts[0], labels[0], int(il[0]), int(ll[0]), mac.SINK_BLANK)
    assert (ref["frames"] == expect).all()
    frames, logp, scores = _mirror(acts, labels, il, ll, mac.SINK_BLANK)
    assert (frames[0] == expect).all(), (frames[0], expect)
    assert float(scores[0]) == np.float32(ref["score"])
    assert (logp[0] == ref["logp"].astype(np.float32)).all()


def test_mirror_on_random_and_planted_lattices():
    rng = np.random.default_rng(11)
    acts, labels, il, ll = mac.random_case(rng, 5, 14, 7, 6, scale=2.0)
    il = np.maximum(il, ll).astype(np.int32)  # feasible
    frames, logp, scores = _mirror(acts, labels, il, ll)
    for b in range(5):
        Tb, Lb = int(il[b]), int(ll[b])
        ref = mac.restate(acts[b], labels[b], Tb, Lb)
        mac.check_valid_path(frames[b], Tb, Lb)
        rescored = mac.score_path(ref["lpb"], ref["lpl"], frames[b, :Lb])
        assert rescored >= ref["score"] - 1e-4 * max(1.0, abs(ref["score"]))
        assert abs(float(scores[b]) - rescored) <= 1e-4 * max(1.0, abs(ref["score"]))
        assert (logp[b, Lb:] == 0).all()
    acts, labels, il, ll, emit = mac.planted_case(rng, 4, 40, 15, 28, gain=20.0)
    frames, logp, scores = _mirror(acts, labels, il, ll)
    for b in range(4):
        Lb = int(ll[b])
        ref = mac.restate(acts[b], labels[b], int(il[b]), Lb)
        assert ref["min_margin"] >= 1e-2
        assert (frames[b, :Lb] == emit[b, :Lb]).all() and (frames[b, Lb:] == -1).all()
        np.testing.assert_allclose(logp[b, :Lb], ref["logp"], rtol=0, atol=1e-5)
        assert abs(float(scores[b]) - ref["score"]) <= 1e-4 * max(1.0, abs(ref["score"]))


# ---- special cases ------------------------------------------------------------------------------------------------------
def test_as_many_labels_as_frames_is_the_single_path():
    rng = np.random.default_rng(1)
    T = 6
    acts, labels, il, ll = mac.random_case(rng, 1, T, T + 1, 5, ragged=False)
    frames, logp, scores = _mirror(acts, labels, il, ll)
    lpb, lpl = mac.cell_logprobs(acts[0], labels[0], T, T, 0)
    assert list(frames[0]) == list(range(T))
    assert abs(float(scores[0]) - sum(lpl[t, t] for t in range(T))) <= 1e-4
    np.testing.assert_allclose(logp[0], [lpl[t, t] for t in range(T)], rtol=0, atol=1e-5)


def test_no_labels_is_the_blank_path():
    rng = np.random.default_rng(2)
    acts, labels, il, ll = mac.random_case(rng, 2, 7, 4, 5, ragged=False, blank=2)
    ll[:] = 0
    il[1] = 5
    frames, logp, scores = _mirror(acts, labels, il, ll, blank=2)
    assert (frames == -1).all() and (logp == 0).all()
    for b in range(2):
        lpb, _ = mac.cell_logprobs(acts[b], labels[b], int(il[b]), 0, 2)
        assert abs(float(scores[b]) - lpb[:, 0].sum()) <= 1e-4
    # U = 1: no label columns at all
    f, lp, s = _mirror(acts[:, :, :1], np.zeros((2, 0), np.int32), il, ll, blank=2)
    assert f.shape == (2, 0) and lp.shape == (2, 0) and (s == scores).all()


def test_one_frame():
    rng = np.random.default_rng(3)
    acts, labels, il, ll = mac.random_case(rng, 2, 1, 2, 4, ragged=False)
    ll[:] = [1, 0]
    frames, logp, scores = _mirror(acts, labels, il, ll)
    lpb, lpl = mac.cell_logprobs(acts[0], labels[0], 1, 1, 0)
    assert frames[0, 0] == 0 and abs(float(scores[0]) - lpl[0, 0]) <= 1e-5 and abs(logp[0, 0] - lpl[0, 0]) <= 1e-5
    lpb, _ = mac.cell_logprobs(acts[1], labels[1], 1, 0, 0)
    assert frames[1, 0] == -1 and logp[1, 0] == 0 and abs(float(scores[1]) - lpb[0, 0]) <= 1e-5


def test_more_labels_than_frames_has_no_path():
    rng = np.random.default_rng(4)
    acts, labels, il, ll = mac.random_case(rng, 3, 8, 7, 4, ragged=False)
    il[1], ll[1] = 3, 5
    frames, logp, scores = _mirror(acts, labels, il, ll)
    assert scores[1] == -np.inf and (frames[1] == -1).all() and (logp[1] == 0).all()
    assert np.isfinite(scores[[0, 2]]).all() and not np.isnan(logp).any()
    assert mac.restate(acts[1], labels[1], 3, 5)["score"] == -np.inf
    alone = _mirror(acts[:1], labels[:1], il[:1], ll[:1])
    for k, got in enumerate((frames, logp, scores)):
        assert got[0].tobytes() == alone[k][0].tobytes()


def test_out_of_range_lengths_are_contained():
    rng = np.random.default_rng(13)
    acts, labels, il, ll = mac.random_case(rng, 6, 12, 6, 8, ragged=False)
    good = _mirror(acts, labels, il, ll)
    il2, ll2 = il.copy(), ll.copy()
    il2[1], ll2[2], il2[3], ll2[4] = 0, 6, 13, -1
    frames, logp, scores = _mirror(acts, labels, il2, ll2)
    assert np.isnan(scores[1:5]).all() and (frames[1:5] == -1).all() and (logp[1:5] == 0).all()
    for b in (0, 5):
        for k, got in enumerate((frames, logp, scores)):
            assert got[b].tobytes() == good[k][b].tobytes(), (b, k)


# ---- the topology option ------------------------------------------------------------------------------------------------
def _tiny_joint():
    torch.manual_seed(0)
    joint = pkg.JointLoss(8, 16, 6)
    enc, pred = torch.randn(2, 9, 8), torch.randn(2, 4, 8)
    labels = torch.randint(1, 6, (2, 3), dtype=torch.int32)
    return joint, enc, pred, labels, torch.tensor([9, 6], dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32)


def test_a_bad_topology_raises():
    acts = torch.zeros(1, 2, 2, 4)
    args = (acts, torch.ones(1, 1, dtype=torch.int32), torch.tensor([2]), torch.tensor([1]))
    with pytest.raises(ValueError, match="topology"):
        pkg.rnnt_align(*args, topology="bogus")
    joint, enc, pred, labels, il, ll = _tiny_joint()
    with pytest.raises(ValueError, match="topology"):
        pkg.align_joint(joint, enc, pred, labels, il, ll, topology="bogus")


def test_standard_is_the_call_without_the_argument():
    rng = np.random.default_rng(6)
    acts, labels, il, ll = ac.random_case(rng, 3, 10, 5, 6)
    t = [torch.tensor(x) for x in (acts, labels, il, ll)]
    for a, b in zip(pkg.rnnt_align(*t), pkg.rnnt_align(*t, topology="standard")):
        assert a.numpy().tobytes() == b.numpy().tobytes()
    joint, enc, pred, labels, il, ll = _tiny_joint()
    for a, b in zip(pkg.align_joint(joint, enc, pred, labels, il, ll),
                    pkg.align_joint(joint, enc, pred, labels, il, ll, topology="standard")):
        assert a.numpy().tobytes() == b.numpy().tobytes()


def test_align_joint_modified_equals_alignment_of_the_cell_logits():
    joint, enc, pred, labels, il, ll = _tiny_joint()
    want = pkg.rnnt_align(joint.cell_logits(enc, pred).float(), labels, il, ll, blank_label=joint.blank_label, topology="modified")
    for slab in (None, 1, 4):
        got = pkg.align_joint(joint, enc, pred, labels, il, ll, slab_frames=slab, topology="modified")
        assert (got[0] == want[0]).all()
        np.testing.assert_allclose(got[1].numpy(), want[1].numpy(), rtol=0, atol=1e-5)
        np.testing.assert_allclose(got[2].numpy(), want[2].numpy(), rtol=0, atol=1e-4)
    for b in range(2):
        mac.check_valid_path(want[0][b].numpy(), int(il[b]), int(ll[b]))


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_workspace_size(lib):
    n = _lib.modified_align_workspace_bytes(600, 150, 32)
    assert n % 256 == 0
    assert n >= 32 * 600 * 150 * 8 + 32 * 601 * 150 // 8  # {lpb, lpl} per cell, one bit per node
    assert n <= 32 * 600 * 192 * 8 + 32 * (600 // 32 + 1) * 192 * 4 + 512  # ... on a row stride of 64 x 3 columns
    assert _lib.modified_align_workspace_bytes(600, 150, 64) > n
    assert _lib.modified_align_workspace_bytes(10, 1100, 2) > _lib.modified_align_workspace_bytes(10, 1024, 2)
    out = ctypes.c_size_t(0)
    assert lib.get_rnnt_modified_align_workspace_size(0, 150, 32, ctypes.byref(out)) == INVALID
    assert lib.get_rnnt_modified_align_workspace_size(600, 0, 32, ctypes.byref(out)) == INVALID
    assert lib.get_rnnt_modified_align_workspace_size(600, 150, 0, ctypes.byref(out)) == INVALID
    assert lib.get_rnnt_modified_align_workspace_size(600, 150, 32, None) == INVALID
    assert lib.get_rnnt_modified_align_workspace_size(10, 8193, 2, ctypes.byref(out)) == INVALID       # maxU > 8192
    assert lib.get_rnnt_modified_align_workspace_size(1 << 16, 1 << 10, 32, ctypes.byref(out)) == INVALID  # B maxT maxU >= 2^31


def test_argument_validation_needs_no_device(lib):
    fake = ctypes.c_void_p(256)  # never dereferenced: rejected before any launch
    o = _lib.make_options(0, 0, 10, 5)

    def cells(acts=fake, S=10, t0=0, labels=fake, ll=fake, il=fake, V=28, B=4, ws=fake, opts=o):
        return lib.compute_rnnt_modified_align_cells(acts, S, t0, labels, ll, il, V, B, ws, opts)

    def path(frames=fake, logp=fake, scores=fake, ll=fake, il=fake, B=4, ws=fake, opts=o):
        return lib.compute_rnnt_modified_align_path(frames, logp, scores, ll, il, B, ws, opts)

    def whole(acts=fake, labels=fake, ll=fake, il=fake, V=28, B=4, frames=fake, logp=fake, scores=fake, ws=fake, opts=o):
        return lib.compute_rnnt_modified_align(acts, labels, ll, il, V, B, frames, logp, scores, ws, opts)

    for name in ("acts", "labels", "ll", "il", "ws"):  # a NULL pointer
        assert cells(**{name: None}) == INVALID, name
    for name in ("frames", "logp", "scores", "ll", "il", "ws"):
        assert path(**{name: None}) == INVALID, name
    for name in ("acts", "labels", "ll", "il", "frames", "logp", "scores", "ws"):
        assert whole(**{name: None}) == INVALID, name
        if name != "ws":
            assert whole(**{name: ctypes.c_void_p(258)}) == INVALID, name  # not 4-byte aligned
    for call in (cells, path, whole):
        assert call(ws=ctypes.c_void_p(260)) == INVALID               # misaligned workspace
        assert call(B=0) == INVALID
        assert call(opts=_lib.make_options(0, -1, 10, 5)) == INVALID
        assert call(opts=_lib.make_options(0, 0, 10, 8193)) == INVALID  # maxU > 8192
        assert call(opts=_lib.make_options(0, 0, 1 << 16, 1 << 10), B=32) == INVALID  # B maxT maxU >= 2^31
        assert call(opts=_lib.make_options(0, 0, 10, 5, loc=_lib.RNNT_CPU)) == INVALID  # no CPU fallback
    for call in (cells, whole):
        assert call(V=1) == INVALID and call(V=0) == INVALID          # alphabet_size < 2
        assert call(opts=_lib.make_options(0, 28, 10, 5)) == INVALID  # blank outside [0, V)
    assert cells(S=0) == INVALID and cells(t0=-1) == INVALID and cells(S=6, t0=5) == INVALID  # the slab leaves [0, maxT)
