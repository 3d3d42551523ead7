"""Batched greedy decoding, CPU side: the C ABI's argument checks (no device needed), the decode loop's semantics on the torch
route against a restatement of utils/decoding.py per utterance, the batch metric builders, and the step kernel's code object."""
import ctypes

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib, decoding, metrics
from tests.test_frontend import small_model
from tests.test_isa_audit import _find, kernels  # noqa: F401  (module-scoped fixture: the built code objects)


@pytest.fixture(scope="module")
def lib():
    pkg.build()
    return _lib.load()


def test_greedy_argument_validation_needs_no_device(lib):
    fake = ctypes.c_void_p(256)  # never dereferenced: every call below is rejected before any launch
    o = _lib.make_options(0, 0, 10, 1)
    n = ctypes.c_size_t(0)
    assert lib.get_rnnt_greedy_workspace_size(10, 4, 640, 28, 0, ctypes.byref(n)) == 0 and n.value % 256 == 0 and n.value > 0
    assert lib.get_rnnt_greedy_workspace_size(10, 4, 640, 4096, 1, ctypes.byref(n)) == 0
    assert lib.get_rnnt_greedy_workspace_size(10, 4, 640, 28, 0, None) == 2
    for args in ((10, 4, 640, 4096, 0), (10, 4, 704, 64, 0), (10, 4, 96, 28, 0), (10, 4, 768, 4096, 1), (10, 4, 192, 4096, 1),
                 (10, 4, 640, 8193, 1), (0, 4, 640, 28, 0), (10, 0, 640, 28, 0), (10, 4, 640, 28, 2), (10, 4, 640, 28, 0x100)):
        assert lib.get_rnnt_greedy_workspace_size(*args, ctypes.byref(n)) == 2, args

    def begin(enc=fake, fl=fake, ms=None, w2=fake, b2=fake, J=640, V=28, B=4, cap=0, dt=0, ws=fake, opts=o):
        return lib.compute_rnnt_greedy_begin(enc, fl, ms, w2, b2, J, V, B, cap, dt, ws, opts)

    def step(pp=fake, hyps=fake, N=8, hl=fake, sc=fake, em=fake, ad=fake, stats=None, J=640, V=28, B=4, dt=0, ws=fake, opts=o):
        return lib.compute_rnnt_greedy_step(pp, hyps, N, hl, sc, em, ad, stats, J, V, B, dt, ws, opts)

    cpu = _lib.make_options(0, 0, 10, 1, loc=_lib.RNNT_CPU)
    blank_oob = _lib.make_options(0, 28, 10, 1)
    no_frames = _lib.make_options(0, 0, 0, 1)
    misaligned = ctypes.c_void_p(256 + 64)
    for call in (begin, step):
        assert call(opts=cpu) == 2            # device-only library
        assert call(opts=blank_oob) == 2      # blank_label >= alphabet_size
        assert call(opts=no_frames) == 2      # maxT = 0
        assert call(ws=None) == 2
        assert call(ws=misaligned) == 2       # workspace not 256-byte aligned
        assert call(dt=0x100) == 2            # RNNT_VISIT_ALL means nothing here
        assert call(dt=3) == 2
        assert call(J=96) == 2                # f32-grade joint: J a multiple of 64
        assert call(V=4096) == 2              # f32-grade joint: V <= 128
        assert call(J=768, V=4096, dt=1) == 2  # f16 joint: J <= 640
        assert call(B=0) == 2
    assert begin(enc=None) == 2 and begin(fl=None) == 2 and begin(w2=None) == 2 and begin(b2=None) == 2
    assert step(pp=None) == 2 and step(hyps=None) == 2 and step(N=0) == 2 and step(hl=None) == 2 and step(sc=None) == 2
    assert step(em=None) == 2 and step(ad=None) == 2


# ---------------------------------------------------------------------------------------------------------------------------
def restate(model, enc_b, max_len, cap, blank):
    """utils/decoding.py:21-108 on one utterance's encoder frames enc_b [T_b, H]: the stateless prediction network over the
    prefix for every decision; ids, sum of the log-softmax of the decisions, smallest top-2 logit gap met."""
    hyp, score, gap = [0], 0.0, np.inf
    if max_len == 0:
        return [], 0.0, gap
    for i in range(enc_b.shape[0]):
        nf = 0
        while True:
            g = model.prediction(torch.tensor([hyp]))[:, -1:, :]
            y = model.joint.logits(enc_b[None, i : i + 1], g)[0, 0, 0]
            top = torch.topk(y, 2).values
            gap = min(gap, float(top[0] - top[1]))
            k = int(torch.argmax(y))
            score += float(torch.log_softmax(y, -1)[k])
            if k == blank:
                break
            hyp.append(k)
            nf += 1
            if max_len is not None and len(hyp) - 1 >= max_len:
                return hyp[1:], score, gap
            if cap and nf >= cap:
                break
    return hyp[1:], score, gap


@pytest.mark.parametrize("seed,blank,cap,max_length", [(0, 0, None, 12), (1, 3, None, "tensor"), (2, 0, 2, 40), (3, 5, 1, 0)])
def test_batch_loop_matches_per_utterance_restatement(seed, blank, cap, max_length):
    model = small_model(seed).double().eval()
    model.joint.blank_label = blank
    with torch.no_grad():
        model.joint.b2[blank] -= 0.3
    torch.manual_seed(100 + seed)
    B = 6
    mel = torch.randn(B, 24, 8, dtype=torch.float64)
    spec_lengths = torch.tensor([24, 17, 0, 9, 24, 2])
    if max_length == "tensor":
        max_length = torch.tensor([0, 5, 3, 12, 40, 1])
    with torch.no_grad():
        enc = model.encoder(mel)
        frames = pkg.reduced_lengths(spec_lengths, model.hp.time_reduction_factor)
        ids, lengths, scores = decoding.greedy_decode_batch(model, mel, spec_lengths, max_length, cap, check_every=3)
        ids2, lengths2, scores2 = decoding.greedy_search_batch(model, enc, frames, max_length, cap)
    assert ids.dtype == torch.int32 and lengths.dtype == torch.int32 and scores.dtype == torch.float64
    assert torch.equal(ids, ids2) and torch.equal(lengths, lengths2) and torch.equal(scores, scores2)
    assert frames[2] == 0 and lengths[2] == 0 and scores[2] == 0.0  # an utterance without frames
    min_gap = np.inf
    for b in range(B):
        ml = max_length if not isinstance(max_length, torch.Tensor) else int(max_length[b])
        with torch.no_grad():
            want, score, gap = restate(model, enc[b, : int(frames[b])], ml, cap, blank)
        min_gap = min(min_gap, gap)
        n = int(lengths[b])
        assert ids[b, :n].tolist() == want, (seed, b, ids[b, :n].tolist(), want)
        assert not ids[b, n:].any()  # zero padding
        assert abs(float(scores[b]) - score) <= 1e-9 * max(1.0, abs(score)), (seed, b, float(scores[b]), score)
    assert min_gap > 1e-9, f"a near-tie on seed {seed}: pick another seed"
    assert (lengths.sum() > 0) == (not isinstance(max_length, int) or max_length > 0)


def test_batch_loop_without_a_symbol_budget_grows_its_buffer():
    """max_length=None: no bound but the frames (the reference's semantics) -- a buffer that fills up is grown, not truncated."""
    model = small_model(3).double().eval()
    with torch.no_grad():
        model.joint.b2[0] -= 3.0  # blank almost never wins: many symbols per frame
    mel = torch.randn(2, 8, 8, dtype=torch.float64)
    with torch.no_grad():
        enc = model.encoder(mel)
        ids, lengths, _ = decoding.greedy_search_batch(model, enc, torch.tensor([4, 3]), None, 30, check_every=2)
        for b, T_b in enumerate((4, 3)):
            want, _, _ = restate(model, enc[b, :T_b], None, 30, 0)
            assert ids[b, : int(lengths[b])].tolist() == want
    assert int(lengths.max()) > enc.shape[1] + 16  # beyond the first buffer


def test_batch_metric_builders_agree_with_the_per_utterance_ones():
    model = small_model(5).double()
    with torch.no_grad():
        model.joint.b2[0] -= 0.4
    mel = torch.randn(3, 20, 8, dtype=torch.float64)
    y_true = torch.tensor([[3, 4, 5, 0, 0], [7, 7, 2, 9, 1], [1, 0, 0, 0, 0]])
    dec1, decb = decoding.greedy_decode_fn(model), decoding.greedy_decode_batch_fn(model)
    acc1 = np.mean([metrics.build_accuracy_fn(dec1)(mel[b : b + 1], y_true[b : b + 1]) for b in range(3)])
    assert metrics.build_batch_accuracy_fn(decb)(mel, y_true) == pytest.approx(acc1, abs=1e-12)
    vocab = ["", " "] + list("abcdefghij")
    to_text = lambda ids: "".join(vocab[int(i)] for i in ids)  # noqa: E731
    w1 = np.mean([metrics.build_wer_fn(dec1, to_text)(mel[b : b + 1], y_true[b : b + 1]) for b in range(3)])
    assert metrics.build_batch_wer_fn(decb, to_text)(mel, y_true) == pytest.approx(w1, abs=1e-12)


def test_step_kernel_code_object(kernels):  # noqa: F811
    meta, asm = kernels
    for dt in ("Li0E", "Li1E", "Li2E"):
        (k,) = _find(meta, "greedy_step_kernel", dt)
        assert int(meta[k]["private_segment_fixed_size"]) == 0, (k, meta[k])
        (a,) = _find(asm, "greedy_step_kernel", dt)
        assert "v_mfma_f32_32x32x16_f16" in asm[a] and "v_mfma_f32_32x32x2_f32" not in asm[a], k
    for name in ("greedy_update_kernel", "greedy_begin_kernel", "greedy_w2_f16_kernel"):
        (k,) = _find(meta, name)
        assert int(meta[k]["private_segment_fixed_size"]) == 0, (k, meta[k])
