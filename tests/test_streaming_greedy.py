"""Streaming greedy decoding (decoding.StreamingGreedyDecoder, include/rnnt.h compute_rnnt_greedy_stream_*), CPU side: the torch
route's state machine against one-call decoding and greedy_decode_batch under many chunkings and slot schedules, finished
slots, the argument checks of feed, the ragged encoder and prediction-network resets in torch, and the C ABI's argument checks
of the new entry points (no device needed)."""
import ctypes
import random

import pytest
import torch

from rnnt_speech_recognition_amd import _lib, decoding
from rnnt_speech_recognition_amd.decoding import StreamingGreedyDecoder
from rnnt_speech_recognition_amd.joint import EncoderStream, PredictionStep
from tests.test_encoder_stream import _blocks, _encoder
from tests.test_frontend import small_model


def stream_model(seed=5, device="cpu"):
    model = small_model(seed)
    with torch.no_grad():
        model.joint.b2[0] += 1.0  # (an untrained joint: blanks and runs of symbols mixed)
    return model.to(device).eval()


def chunkings(L, f, rng):
    """Chunk lengths covering L frames: one feed, chunks of f, random multiples of f with a ragged final chunk."""
    out = {"one": [L], "f": [f] * (L // f) + ([L % f] if L % f else [])}
    r, left = [], L
    while left > 0:
        c = f * rng.randint(1, 4)
        if c >= left:
            c = left
        r.append(c)
        left -= c
    out["random"] = r
    return out


def one_call(model, x, max_length=None, mpf=None):
    """The stream fed in one call to a 1-slot decoder -> (ids list, length, score)."""
    dec = StreamingGreedyDecoder(model, 1, x.shape[0], max_length=max_length, max_symbols_per_frame=mpf)
    dec.start([0])
    ids, counts = dec.feed(x[None], [x.shape[0]], [True])
    hi, hl, hs = dec.hypotheses()
    assert ids[0, : int(counts[0])].tolist() == hi[0, : int(hl[0])].tolist()
    return hi[0, : int(hl[0])].tolist(), int(hl[0]), hs[0].clone()


def run_schedule(model, streams, S, Tc, plans, max_length=None, mpf=None, seed=0, extra_restart=None):
    """Feed streams through an S-slot decoder.  plans[i] = (slot, start_feed, chunk lengths); a stream starts at its start feed
    (start() before that feed) and takes one chunk per feed, sitting a feed out now and then.  Returns per stream (ids, length,
    score) read right after its final feed, and the ids its feeds emitted, concatenated."""
    rng = random.Random(seed)
    dec = StreamingGreedyDecoder(model, S, Tc, max_length=max_length, max_symbols_per_frame=mpf, check_every=3)
    F = streams[0].shape[1]
    state = [dict(pos=0, k=0, started=False, done=False) for _ in streams]
    results, emitted = {}, {i: [] for i in range(len(streams))}
    feed_no = 0
    while not all(s["done"] for s in state):
        to_start = [i for i, (slot, sf, _) in enumerate(plans) if sf == feed_no]
        if to_start:
            dec.start([plans[i][0] for i in to_start])
            for i in to_start:
                state[i]["started"] = True
        if extra_restart is not None and extra_restart[0] == feed_no:
            dec.start([extra_restart[1]])
        mel = torch.randn(S, Tc, F, dtype=streams[0].dtype, device=streams[0].device)  # (garbage past each slot's frames)
        frames, final = [0] * S, [False] * S
        owner = {}
        for i, (slot, _, chunks) in enumerate(plans):
            st = state[i]
            if not st["started"] or st["done"] or (feed_no % 3 == 1 and rng.random() < 0.5):
                continue  # not yet started, finished, or sitting this feed out
            c = chunks[st["k"]]
            mel[slot, :c] = streams[i][st["pos"]: st["pos"] + c]
            frames[slot], final[slot] = c, st["k"] == len(chunks) - 1
            owner[slot] = i
            st["pos"] += c
            st["k"] += 1
        ids, counts = dec.feed(mel, frames, final)
        for slot, i in owner.items():
            emitted[i] += ids[slot, : int(counts[slot])].tolist()
            if final[slot]:
                state[i]["done"] = True
                hi, hl, hs = dec.hypotheses()
                results[i] = (hi[slot, : int(hl[slot])].tolist(), int(hl[slot]), hs[slot].clone())
        feed_no += 1
    return results, emitted


def _streams(model, lengths, seed):
    torch.manual_seed(seed)
    F = model.encoder.input_norm.num_features
    return [torch.randn(L, F) for L in lengths]


@pytest.mark.parametrize("mpf", [None, 3])
def test_chunked_streams_equal_one_call_and_the_batch_decoder(mpf):
    model = stream_model()
    f = model.encoder.reduce.factor
    lengths = [30, 25, 17, 9, 22]
    X = _streams(model, lengths, 1)
    want = [one_call(model, x, 40, mpf) for x in X]
    for x, (ids, n, score) in zip(X, want):  # property 2 on the torch route
        bi, bl, bs = decoding.greedy_decode_batch(model, x[None], None, 40, mpf)
        assert bi[0, : int(bl[0])].tolist() == ids
        assert abs(float(bs[0]) - float(score)) <= 1e-4 * max(1.0, abs(float(score)))
    assert sum(n for _, n, _ in want) >= 10
    rng = random.Random(7)
    for kind in ["one", "f", "random"]:
        plans = []
        for i, L in enumerate(lengths):
            chunks = chunkings(L, f, rng)[kind]
            plans.append(([1, 3, 5, 0, 2][i], i, chunks))  # slot 4 idles throughout; staggered starts
        Tc = max(max(p[2]) for p in plans)
        got, emitted = run_schedule(model, X, 6, Tc, plans, 40, mpf, seed=len(kind))
        for i in range(len(X)):
            ids, n, score = got[i]
            assert ids == want[i][0] and n == want[i][1], (kind, i)
            assert emitted[i] == ids
            # the torch route sums in torch's order: to rounding (the engine is bitwise: tests/test_streaming_greedy_gpu.py)
            assert abs(float(score) - float(want[i][2])) <= 1e-5 * max(1.0, abs(float(want[i][2]))), (kind, i)


def test_a_slot_restarted_mid_stream_decodes_its_new_stream():
    model = stream_model()
    X = _streams(model, [24, 20], 2)
    want = one_call(model, X[1], 40)
    # stream 0 in slot 2 for two feeds, then slot 2 restarted with stream 1 (stream 0 never finishes there)
    dec = StreamingGreedyDecoder(model, 3, 8, max_length=40, check_every=2)
    dec.start([2])
    F = X[0].shape[1]
    for k in range(2):
        mel = torch.zeros(3, 8, F)
        mel[2] = X[0][8 * k: 8 * k + 8]
        dec.feed(mel, [0, 0, 8], [False] * 3)
    dec.start(torch.tensor([False, False, True]))
    ids, n, _ = dec.hypotheses()
    assert int(n[2]) == 0 and int(ids[2].abs().sum()) == 0
    for k, c in enumerate([8, 8, 4]):
        mel = torch.zeros(3, 8, F)
        mel[2, :c] = X[1][8 * k: 8 * k + c]
        dec.feed(mel, [0, 0, c], [False, False, k == 2])
    ids, n, sc = dec.hypotheses()
    assert ids[2, : int(n[2])].tolist() == want[0]
    assert abs(float(sc[2]) - float(want[2])) <= 1e-5 * max(1.0, abs(float(want[2])))


def test_finished_slots_emit_nothing():
    model = stream_model()
    X = next(x for x in (_streams(model, [12], k) for k in range(20)) if one_call(model, x[0], 40)[1] > 0)
    dec = StreamingGreedyDecoder(model, 2, 12, max_length=40)
    F = X[0].shape[1]
    ids, counts = dec.feed(torch.randn(2, 12, F), [12, 12], [False, False])  # no stream started: every slot is finished
    assert counts.tolist() == [0, 0] and ids.shape == (2, 0)
    dec.start([0])
    mel = torch.zeros(2, 12, F)
    mel[0] = X[0]
    dec.feed(mel, [12, 0], [True, False])
    before = dec.hypotheses()
    assert int(before[1][0]) > 0
    ids, counts = dec.feed(torch.randn(2, 12, F), [12, 12], [False, True])
    assert counts.tolist() == [0, 0]
    after = dec.hypotheses()
    assert all(torch.equal(p, q) for p, q in zip(before, after))
    # a spent budget finishes a stream too
    dec = StreamingGreedyDecoder(model, 1, 12, max_length=1)
    dec.start([0])
    _, c1 = dec.feed(X[0][None], [12], [False])
    _, c2 = dec.feed(X[0][None], [12], [False])
    assert int(c1[0]) == 1 and int(c2[0]) == 0


def test_feed_checks_its_arguments():
    model = stream_model()
    f = model.encoder.reduce.factor
    F = model.encoder.input_norm.num_features
    dec = StreamingGreedyDecoder(model, 2, 8, max_length=10)
    dec.start([0, 1])
    with pytest.raises(ValueError):
        dec.feed(torch.zeros(2, 8, F), [f + 1, 0], [False, False])  # non-final, not a multiple of f
    dec.feed(torch.zeros(2, 8, F), [f + 1, 0], [True, False])       # (final: any length)
    with pytest.raises(ValueError):
        dec.feed(torch.zeros(2, 9, F), [8, 8], [False, False])      # Tc > max_chunk_frames
    with pytest.raises(ValueError):
        dec.feed(torch.zeros(3, 8, F), [8, 8, 8], [False] * 3)      # wrong slot count
    with pytest.raises(ValueError):
        dec.feed(torch.zeros(2, 8, F + 1), [8, 8], [False, False])  # wrong feature width
    with pytest.raises(ValueError):
        dec.feed(torch.zeros(2, 8, F), [8, 9], [False, True])       # more frames than the chunk has
    with pytest.raises(ValueError):
        dec.feed(torch.zeros(2, 8, F), [8], [False])                 # frames of the wrong length
    with pytest.raises(ValueError):
        StreamingGreedyDecoder(model, 0, 8)
    with pytest.raises(ValueError):
        StreamingGreedyDecoder(model, 1025, 8)
    with pytest.raises(ValueError):
        dec.start([2])


def test_ragged_torch_encoder_rows_equal_their_own_runs():
    enc = _encoder(4, ridx=1, f=2)
    R, F = 4, enc.input_norm.num_features
    x = torch.randn(R, 10, F)
    es = EncoderStream(enc)
    es.begin(R, 10)
    es.run(x[:, :4])  # some state
    rows = [10, 0, 7, 4]
    out = es.run(x, row_frames=rows, reset=[False, False, True, False])
    st = es.state()
    for r, n in enumerate(rows):
        one = EncoderStream(enc)
        one.begin(1, 10)
        if r != 2:
            one.run(x[r: r + 1, :4])
        if n:
            want = one.run(x[r: r + 1, :n])
            torch.testing.assert_close(out[r: r + 1, : want.shape[1]], want, rtol=1e-5, atol=1e-6)
            assert int(out[r, want.shape[1]:].abs().sum()) == 0
        for (h, c), (h1, c1) in zip(st, one.state()):
            torch.testing.assert_close(h[r], h1[0], rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(c[r], c1[0], rtol=1e-5, atol=1e-6)


def test_torch_prediction_reset_restarts_only_its_rows():
    model = stream_model()
    ps = PredictionStep(model.prediction, model.joint.W1)
    fresh = ps.begin(4).clone()
    ps.step(torch.tensor([3, -1, 5, 2], dtype=torch.int32))
    moved = ps.step(torch.tensor([1, 4, -1, 2], dtype=torch.int32)).clone()
    pp = ps.reset(torch.tensor([True, False, False, True]))
    assert torch.equal(pp[0], fresh[0]) and torch.equal(pp[3], fresh[3])
    assert torch.equal(pp[1], moved[1]) and torch.equal(pp[2], moved[2])


def test_stream_argument_validation_needs_no_device():
    lib = _lib.load()
    INV, OK = 2, 0
    n = ctypes.c_size_t(0)
    # (max_chunk_frames, slots, enc_width, joint_size, alphabet_size, joint_dtype)
    assert lib.get_rnnt_greedy_stream_workspace_size(16, 64, 640, 640, 4096, 1, ctypes.byref(n)) == OK
    big = n.value
    assert lib.get_rnnt_greedy_workspace_size(16, 64, 640, 4096, 1, ctypes.byref(n)) == OK and n.value < big
    for args in [(0, 4, 64, 64, 12, 0),        # no frames
                 (8, 0, 64, 64, 12, 0),        # no slots
                 (8, 1025, 64, 64, 12, 0),     # too many slots
                 (8, 4, 0, 64, 12, 0),         # no encoder width
                 (8, 4, 4097, 64, 12, 0),      # encoder too wide
                 (8, 4, 64, 64, 0, 0),         # no vocabulary
                 (8, 4, 64, 100, 12, 1),       # f16 joint size not a multiple of 128
                 (8, 4, 64, 64, 12, 2)]:       # joint_dtype
        assert lib.get_rnnt_greedy_stream_workspace_size(*args, ctypes.byref(n)) == INV, args
    assert lib.get_rnnt_greedy_stream_workspace_size(8, 4, 64, 64, 12, 0, None) == INV
    ws, p = 0x10000, 0x1000
    opts = _lib.make_options(0, 0, 8, 1)
    begin = lambda W1=p, ws=ws, opts=opts, S=4, V=12: lib.compute_rnnt_greedy_stream_begin(  # noqa: E731
        W1, p, p, p, 64, 64, V, S, 0, ws, opts)
    assert begin(W1=None) == INV
    assert begin(ws=None) == INV
    assert begin(ws=ws + 64) == INV                                   # workspace not 256-byte aligned
    assert begin(S=0) == INV
    assert begin(S=1025) == INV
    assert begin(opts=_lib.make_options(0, 0, 0, 1)) == INV          # maxT = max_chunk_frames = 0
    assert begin(opts=_lib.make_options(0, 12, 8, 1)) == INV         # blank beyond the vocabulary
    assert begin(opts=_lib.make_options(0, 0, 8, 1, loc=0)) == INV   # loc = CPU
    feed = lambda enc=p, Te=8, fr=p, out=p, ws=ws: lib.compute_rnnt_greedy_stream_feed(  # noqa: E731
        enc, Te, fr, None, None, None, 0, out, out, out, 64, 64, 12, 4, 0, ws, opts)
    assert feed(fr=None) == INV
    assert feed(out=None) == INV
    assert feed(Te=9) == INV                                          # more encoder frames than max_chunk_frames
    assert feed(Te=-1) == INV
    assert feed(enc=None) == INV                                      # frames but no encoder output
    assert feed(ws=None) == INV
    blocks = _blocks([(16, 16, False)])
    reset = lambda r=p, out=p, rows=4, ws=ws: lib.compute_rnnt_prednet_reset(  # noqa: E731
        r, out, blocks, 1, 8, 12, 64, rows, ws, opts)
    assert reset(r=None) == INV
    assert reset(out=None) == INV
    assert reset(out=p + 4) == INV                                    # misaligned
    assert reset(rows=0) == INV
    assert reset(rows=1025) == INV
    assert reset(ws=ws + 64) == INV
    good = _blocks([(64, 32, True), (64, 32, True), (64, 64, False)])
    rows = lambda x=0x3000, frames=50, rf=p, out=0x4000, ws=ws: lib.compute_rnnt_encoder_run_rows(  # noqa: E731
        x, frames, rf, None, out, good, 3, 24, 1e-3, 1, 2, 16, 100, ws, opts)
    assert rows(rf=None) == INV
    assert rows(x=None) == INV
    assert rows(out=0x4004) == INV
    assert rows(frames=0) == INV
    assert rows(frames=101) == INV
    assert rows(ws=None) == INV
