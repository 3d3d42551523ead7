"""Per-token emission frames and log-probabilities (include/rnnt.h, "timed decoding"), CPU side: the torch mirror of the four
decoders with token_times=True against the float64 restatements of tests/token_time_cases.py on the scripted scenarios of
tests/decode_scripts.py (frames exactly, log-probabilities within one decision's score bar); the survivor of a merge keeps its
own frames; the timed stable length; chunked streams against one call, a reset restarting at frame 0; words with times and
confidences; and the argument checks of the new entry points (no device needed)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib, decoding, joint as jmod
from rnnt_speech_recognition_amd.decoding import StreamingBeamDecoder, StreamingGreedyDecoder, timed_words
from rnnt_speech_recognition_amd.features import CharEncoder
from tests import decode_scripts as ds
from tests import token_time_cases as tt
from tests.test_decode_scripts import MirrorBeam, MirrorGreedy, _joint_module, _script_logits
from tests.test_streaming_beam import LENGTHS, SLOTS, beam_model, plans_for
from tests.test_streaming_greedy import _streams, stream_model


class TimedMirrorBeam(MirrorBeam):
    def __init__(self, sc):
        self.sc, self.sj = sc, sc.joint
        self.bj = jmod.BeamJoint(_joint_module(self.sj, sc.blank), beam=sc.K, token_times=True)
        assert not self.bj.engine

    def results(self):
        hyps, lengths, scores, self.frames, self.logp = (x.numpy() for x in self.bj.results())
        return hyps, lengths, scores


class TimedMirrorGreedy(MirrorGreedy):
    def __init__(self, sc):
        self.sc, self.sj = sc, sc.joint
        self.gj = jmod.GreedyJoint(_joint_module(self.sj, sc.blank), token_times=True)
        assert not self.gj.engine

    def grow(self, max_hyp_len):
        g = self.gj
        while g.hyps.shape[1] < max_hyp_len:
            g.grow_hyps()  # (all three buffers)
        g.hyps, g.frames, g.logp = g.hyps[:, :max_hyp_len].clone(), g.frames[:, :max_hyp_len].clone(), g.logp[:, :max_hyp_len].clone()


def _beam(sc, steps=None):
    if steps is not None:
        sc.steps = steps
    eng, untimed = TimedMirrorBeam(sc), MirrorBeam(sc)
    args = (sc.joint, sc.script, sc.B, sc.K, sc.frames, sc.maxT, sc.blank, sc.steps, _script_logits(sc), sc.ties_allowed)
    trace, ref, _, _ = ds.run_beam(eng, *args)
    plain = ds.run_beam(untimed, *args)[0]
    assert ds.traces_equal(trace, plain), "token_times changed ids, lengths, scores, parents or emitted"
    want = tt.restate_beam(sc, _script_logits(sc))
    assert [[y for y, _ in b] for b in want.beams] == [[y for y, _ in b] for b in ref.beams]
    err, bar = tt.check_beam_times(sc, want, trace[-1][1], eng.frames, eng.logp)
    print(f"[{sc.name}] frames exact; worst log-probability error {err:.3e} (bar {bar:.3e})")
    return eng, want


def _greedy(sc):
    eng = TimedMirrorGreedy(sc)
    args = (sc.joint, sc.script, sc.B, sc.frames, sc.max_symbols, sc.max_per_frame, sc.maxT, sc.blank, sc.hyp_lens,
            _script_logits(sc), sc.ties_allowed)
    trace, ref, _, _ = ds.run_greedy(eng, *args)
    plain = ds.run_greedy(MirrorGreedy(sc), *args)[0]
    assert ds.traces_equal(trace, plain), "token_times changed ids, lengths, scores, emitted or all_done"
    want = tt.restate_greedy(sc, _script_logits(sc))
    assert want.y == ref.y
    err, bar = tt.check_greedy_times(sc, want, eng.gj.frames.numpy(), eng.gj.logp.numpy())
    print(f"[{sc.name}] frames exact; worst log-probability error {err:.3e} (bar {bar:.3e})")
    return eng, want


# ---- beam search ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 5, 8, 16])
def test_forced_merges_keep_the_survivors_frames(K):
    sc = ds.merge_scenario(K)
    eng, want = _beam(sc)
    assert want.ev.merges >= 4
    # a merged hypothesis arrived by an emission at the merge frame (the short parent, first-ranked) and by a blank (the long one,
    # whose last token is a frame older): the survivor's last frame must be the merge frame itself
    hit = 0
    for b in range(sc.B):
        for k, row in enumerate(want.times[b]):
            if row and row[-1][0] == min(sc.steps, want.Tb[b]) - 1 and (min(sc.steps, want.Tb[b]) - 1) % 2 == 0:
                assert eng.frames[b, k, len(row) - 1] == row[-1][0]
                hit += 1
    assert hit, "no hypothesis ends on a merge frame: the scenario does not show which member's frames were kept"


def test_the_first_ranked_member_of_a_merge_keeps_its_frame():
    sc = tt.late_twin_scenario()
    eng, want = _beam(sc, steps=2)
    a = 1
    assert [y for y, _ in want.beams[0]][:2] == [(a,), (a, 2)] and want.ev.merges == 1
    # (a) arrived as () + a at frame 1 (first-ranked) and as (a) + blank with its a from frame 0: frame 1 wins
    assert eng.frames[0, 0, 0] == 1 and eng.frames[0, 1, :2].tolist() == [0, 1]
    assert abs(float(eng.logp[0, 0, 0]) - want.times[0][0][0][1]) <= 1e-6
    # the score is the sum over both members, so it is larger than the kept path's own log-probability
    path = want.times[0][0][0][1] + math.log(1.0 / (1.0 + math.exp(-0.4) + np.exp(-9.0 - 0.2 * np.arange(2, 9)).sum()))
    assert want.beams[0][0][1] > path + 0.2


def test_timed_stable_length_lags_and_catches_up():
    sc = tt.late_twin_scenario()
    ref = tt.TimedBeamRestatement(_script_logits(sc), sc.B, sc.K, sc.frames, sc.maxT, sc.blank)
    seen = []
    for _ in range(sc.steps):
        ref.step()
        toks = [list(y) for y, _ in ref.beams[0]]
        stable = 0
        while all(stable < len(y) for y in toks) and all(y[stable] == toks[0][stable] for y in toks):
            stable += 1
        seen.append((stable, ref.timed_stable(0)))
    assert all(t <= s for s, t in seen)
    assert any(t < s for s, t in seen), seen   # tokens shared, frames not
    assert seen[-1][1] >= 1, seen  # one ancestor took the beam over: the shared token's time is final now
    _beam(sc)


@pytest.mark.parametrize("K", [1, 2, 3, 5, 8, 16])
def test_exact_ties(K):
    sc = ds.tie_scenario(K)
    eng, want = _beam(sc)
    if K >= 2:  # the two tied symbols of frame 0 hold slots 0 and 1 of a one-frame decode, both emitted at frame 0
        e1, w1 = _beam(ds.tie_scenario(K), steps=1)
        assert e1.frames[0, 0, 0] == 0 and e1.frames[0, 1, 0] == 0 and e1.logp[0, 0, 0] == e1.logp[0, 1, 0]


def test_random_script_with_a_vocabulary_smaller_than_the_beam():
    _beam(ds.small_vocabulary_scenario())


def test_full_beam_of_16():
    _beam(ds.full_beam_scenario())


def test_nothing_taken_carries_the_times_over():
    _beam(ds.nothing_taken_scenario())


# ---- greedy --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, 1, 2, 3])
def test_greedy_symbol_caps(cap):
    sc = ds.greedy_caps_scenario(cap)
    eng, want = _greedy(sc)
    for b in range(sc.B):  # at most `cap` tokens carry one frame
        fr = [f for f, _ in want.times[b]]
        assert fr == sorted(fr) and (cap <= 0 or max([fr.count(f) for f in fr], default=0) <= cap)


def test_greedy_batch_of_257():
    _greedy(ds.greedy_batch_scenario(257))


def test_greedy_pause_and_resume_carries_frames_and_logp():
    small, _ = _greedy(ds.greedy_pause_scenario([3, 5, 40]))
    large, _ = _greedy(ds.greedy_pause_scenario([40]))
    assert np.array_equal(small.gj.frames.numpy(), large.gj.frames.numpy())
    assert small.gj.logp.numpy().tobytes() == large.gj.logp.numpy().tobytes()


@pytest.mark.parametrize("dtype", [0, 1])
def test_greedy_exact_argmax_ties_pin_the_frames(dtype):
    sc = ds.greedy_tie_scenario(dtype)
    eng, want = _greedy(sc)
    assert want.ev.ties >= 8
    # row 0, by the script: frame 0 ties (s0, s2) -> s0 twice (the cap of 2), frame 1 ties (blank, s3) -> blank, frame 2 ties
    # (s1, blank) -> s1 twice, frame 3 ties (s2, s3) -> s2 twice, and again from frame 4
    s0, s1, s2, _ = (3, 7, 70, 101) if dtype else (2, 5, 13, 27)
    assert list(want.y[0][:6]) == [s0, s0, s1, s1, s2, s2]
    assert eng.gj.frames[0, :8].tolist() == [0, 0, 2, 2, 3, 3, 4, 4]


# ---- streams on the torch mirror -----------------------------------------------------------------------------------------------
def test_streaming_greedy_frames_count_from_the_reset_across_chunks():
    model = stream_model()
    f = model.encoder.reduce.factor
    X = _streams(model, LENGTHS[:5], 1)

    def one(x):
        dec = StreamingGreedyDecoder(model, 1, x.shape[0], max_length=40, token_times=True)
        dec.start([0])
        dec.feed(x[None], [x.shape[0]], [True])
        return tt.read_timed_greedy(dec, 0)

    want = [one(x) for x in X]
    assert sum(len(w[0]) for w in want) >= 10 and any(w[1] and w[1][-1] >= 4 for w in want)
    # the batch decoder agrees on ids and frames
    for x, w in zip(X, want):
        ids, n, _, frames, logp = decoding.greedy_decode_batch(model, x[None], None, 40, token_times=True)
        assert ids[0, : int(n[0])].tolist() == w[0] and frames[0, : int(n[0])].tolist() == w[1]
    for kind in ["f", "random"]:
        plans, Tc = plans_for(LENGTHS[:5], f, kind, 5, SLOTS)
        dec = StreamingGreedyDecoder(model, 16, Tc, max_length=40, check_every=3, token_times=True)
        got = tt.run_streams(dec, X, plans, tt.read_timed_greedy, seed=3, extra_restart=(2, 11))
        for i, w in enumerate(want):
            assert got[i][0] == w[0] and got[i][1] == w[1], (kind, i)
            assert np.allclose(np.frombuffer(got[i][2], np.float32), np.frombuffer(w[2], np.float32), atol=1e-5)
    # a slot that is started again: its frames restart at 0
    dec = StreamingGreedyDecoder(model, 2, 32, max_length=40, token_times=True)
    for x in (X[0], X[1]):
        dec.start([1])
        mel = torch.zeros(2, 32, x.shape[1])
        mel[1, : x.shape[0]] = x
        dec.feed(mel, [0, x.shape[0]], [False, True])
        r = tt.read_timed_greedy(dec, 1)
        assert r[:2] == want[0 if x is X[0] else 1][:2]


@pytest.mark.parametrize("K", [1, 4])
def test_streaming_beam_times_and_timed_stable_lengths(K):
    model = beam_model()
    f = model.encoder.reduce.factor
    X = _streams(model, LENGTHS[:5], 1)
    X = [x.double() for x in X]

    def one(x):
        dec = StreamingBeamDecoder(model, 1, x.shape[0], beam=K, max_length=24, token_times=True)
        dec.start([0])
        dec.feed(x[None], [x.shape[0]], [True])
        return tt.read_timed_beam(dec, 0)

    want = [one(x) for x in X]
    plans, Tc = plans_for(LENGTHS[:5], f, "random", 5, SLOTS)
    final = {}

    def finality(dec, owner):  # what lies below the timed stable length never changes again
        ids, _, _, frames, _ = dec.timed_nbest()
        tst, st = dec.timed_stable_lengths(), dec.bj.results()[3]
        for slot, i in owner.items():
            n = int(tst[slot])
            assert n <= int(st[slot])
            pairs = list(zip(ids[slot, 0, :n].tolist(), frames[slot, 0, :n].tolist()))
            old = final.get(i, [])
            assert pairs[: len(old)] == old, (i, old, pairs)
            final[i] = pairs if len(pairs) > len(old) else old

    dec = StreamingBeamDecoder(model, 16, Tc, beam=K, max_length=24, token_times=True)
    got = tt.run_streams(dec, X, plans, tt.read_timed_beam, seed=3, extra_restart=(2, 11), after_feed=finality)
    for i, w in enumerate(want):
        assert [r[:2] for r in got[i][0]] == [r[:2] for r in w[0]] and got[i][1:] == w[1:], i
    # untimed twin on the mirror: the same ids and scores
    plain = StreamingBeamDecoder(model, 1, X[0].shape[0], beam=K, max_length=24)
    plain.start([0])
    plain.feed(X[0][None], [X[0].shape[0]], [True])
    ids, lengths, scores = plain.nbest()
    assert [ids[0, k, : int(lengths[0, k])].tolist() for k in range(len(want[0][0]))] == [r[0] for r in want[0][0]]


def test_timed_methods_need_token_times():
    model = stream_model()
    with pytest.raises(RuntimeError, match="token_times"):
        StreamingGreedyDecoder(model, 1, 8).timed_hypotheses()
    dec = StreamingBeamDecoder(beam_model(), 1, 8, beam=2)
    for name in ("timed_hypotheses", "timed_nbest", "timed_stable_lengths"):
        with pytest.raises(RuntimeError, match="token_times"):
            getattr(dec, name)()


# ---- words ---------------------------------------------------------------------------------------------------------------------
def test_words_with_times_confidences_and_the_final_count():
    enc = CharEncoder()
    ids = enc.encode("hi the re")
    frames = [2, 3, 5, 9, 9, 10, 14, 20, 21]
    logp = [-0.1, -0.7, -0.05, -0.2, -0.3, -0.01, -2.0, -0.4, -0.5]
    sec = 0.06
    words, final = timed_words(ids, frames, logp, enc, sec, stable_tokens=6)
    assert [w[0] for w in words] == ["hi", "the", "re"] and final == 2  # "re" (tokens 7, 8) lies beyond the 6 stable tokens
    assert [round(w[1] / sec) for w in words] == [2, 9, 20] and [round(w[2] / sec) for w in words] == [4, 11, 22]
    assert words[0][1] == 2 * sec and words[0][2] == (3 + 1) * sec
    # the weakest token of the word; the spaces (-0.05, -2.0) belong to no word (log-probabilities are f32: 2^-24 relative)
    assert [w[3] for w in words] == pytest.approx([math.exp(-0.7), math.exp(-0.3), math.exp(-0.5)], rel=2e-7, abs=0)
    assert timed_words(ids, frames, logp, enc, sec)[1] == 3                      # greedy: everything reported is final
    assert timed_words(ids, frames, logp, enc, sec, stable_tokens=4)[1] == 1     # "the" only half stable
    assert timed_words([], [], [], enc, sec) == ([], 0)


@pytest.mark.parametrize("beam", [None, 4])
def test_transcriber_words_on_the_torch_route(beam):
    from rnnt_speech_recognition_amd import alignment
    from tests import frontend_cases as fc
    from tests.test_frontend import small_model

    model = small_model(3).eval()
    hp, sr = model.hp, 16000
    audio = fc.signal(1.0, sr, seed=21)
    enc = CharEncoder(["", " "] + list("abcdefghij"))  # the model's 12 symbols: the blank, a space, ten letters
    kw = dict(max_length=40, max_symbols_per_frame=3) if beam is None else {}
    tr = decoding.StreamingTranscriber(model, hp, sr, 2, len(audio), beam=beam, token_times=True, **kw)
    tr.start([0, 1])
    au = torch.zeros(2, len(audio))
    au[1] = torch.tensor(audio)
    tr.feed(au, [0, len(audio)], [False, False])  # (not final: a beam may still disagree on its tail)
    words, final = tr.words(1, enc)
    ids, frames, logp = (x[1] for x in tr.decoder.timed_hypotheses())
    n = int((frames >= 0).sum())
    assert n >= 3 and words, (n, words)
    sec = alignment.frame_seconds(hp, sr)
    stable = int(tr.decoder.timed_stable_lengths()[1]) if beam is not None else None
    assert (words, final) == timed_words(ids[:n], frames[:n], logp[:n], enc, sec, stable)
    spans = alignment.word_times(ids[:n], frames[:n], enc)
    assert [(w, round(s / sec), round(e / sec) - 1) for w, s, e, _ in words] == spans
    assert all(0.0 < c <= 1.0 and e > s >= 0.0 for _, s, e, c in words) and 0 <= final <= len(words)
    if beam is None:
        assert final == len(words)  # greedy never rewrites
    assert tr.words(0, enc) == ([], 0)  # a slot that was fed nothing
    assert len(tr.words(1)[0]) >= 1    # the default vocabulary (CharEncoder())
    plain = decoding.StreamingTranscriber(model, hp, sr, 1, 3000, beam=beam, **kw)
    with pytest.raises(RuntimeError, match="token_times"):
        plain.words(0, enc)


# ---- the boundary of the C ABI -------------------------------------------------------------------------------------------------
def test_argument_validation_needs_no_device():
    pkg.build()
    lib = _lib.load()
    fake, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)  # never dereferenced: every call below is rejected before any launch
    o = _lib.make_options(0, 0, 8, 1)
    n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
    # sizes: the untimed queries answer what they answered; the timed ones add 4 S K N words
    assert lib.get_rnnt_beam_workspace_size(50, 8, 4, 640, 4096, 1, ctypes.byref(n)) == 0
    assert lib.get_rnnt_beam_timed_workspace_size(50, 8, 4, 640, 4096, 1, ctypes.byref(m)) == 0
    assert m.value % 256 == 0 and 0 <= m.value - n.value - 4 * 8 * 4 * 50 * 4 < 256
    assert lib.get_rnnt_beam_stream_workspace_size(8, 16, 4, 100, 640, 640, 4096, 1, ctypes.byref(n)) == 0
    assert lib.get_rnnt_beam_stream_timed_workspace_size(8, 16, 4, 100, 640, 640, 4096, 1, ctypes.byref(m)) == 0
    assert m.value % 256 == 0 and 0 <= m.value - n.value - 4 * 16 * 4 * 100 * 4 < 256
    assert lib.get_rnnt_beam_timed_workspace_size(50, 8, 4, 640, 4096, 1, None) == 2
    assert lib.get_rnnt_beam_timed_workspace_size(50, 8, 4, 640, 4096, 0x101, ctypes.byref(m)) == 2
    # 6 S K N < 2^31: a stream the untimed layout takes and the timed one refuses
    big = (1 << 31) // (6 * 1024) + 1
    assert lib.get_rnnt_beam_stream_workspace_size(8, 64, 16, big, 640, 640, 28, 0, ctypes.byref(n)) == 0
    assert lib.get_rnnt_beam_stream_timed_workspace_size(8, 64, 16, big, 640, 640, 28, 0, ctypes.byref(m)) == 2
    assert lib.get_rnnt_beam_stream_timed_workspace_size(8, 64, 16, big - 1, 640, 640, 28, 0, ctypes.byref(m)) == 0

    def gstep(pp=fake, h=fake, hf=fake, hl=fake, N=16, n_=fake, sc=fake, em=fake, ad=fake, st=None, fb=None, J=640, V=28, B=8, dt=0,
              ws=fake, opts=o):
        return lib.compute_rnnt_greedy_step_timed(pp, h, hf, hl, N, n_, sc, em, ad, st, fb, J, V, B, dt, ws, opts)

    def gfeed(enc=fake, Te=8, cf=fake, rs=None, fi=None, ms=None, mpf=0, n_=fake, sc=fake, ad=fake, fb=fake, H=640, J=640, V=28, S=8,
              dt=0, ws=fake, opts=o):
        return lib.compute_rnnt_greedy_stream_feed_timed(enc, Te, cf, rs, fi, ms, mpf, n_, sc, ad, fb, H, J, V, S, dt, ws, opts)

    def bbegin(ep=fake, fl=fake, w2=fake, b2=fake, J=640, V=28, B=8, K=4, dt=0, ws=fake, opts=o):
        return lib.compute_rnnt_beam_timed_begin(ep, fl, w2, b2, J, V, B, K, dt, ws, opts)

    def bstep(pp=fake, par=fake, em=fake, tl=None, ts=None, lse=None, J=640, V=28, B=8, K=4, dt=0, ws=fake, opts=o):
        return lib.compute_rnnt_beam_timed_step(pp, par, em, tl, ts, lse, J, V, B, K, dt, ws, opts)

    def bres(h=fake, n_=fake, sc=fake, hf=fake, hl=fake, J=640, V=28, B=8, K=4, dt=0, ws=fake, opts=o):
        return lib.compute_rnnt_beam_timed_results(h, n_, sc, hf, hl, J, V, B, K, dt, ws, opts)

    def sbegin(w1=fake, b1=fake, w2=fake, b2=fake, H=640, J=640, V=28, S=16, K=4, N=100, dt=0, ws=fake, opts=o):
        return lib.compute_rnnt_beam_stream_timed_begin(w1, b1, w2, b2, H, J, V, S, K, N, dt, ws, opts)

    def sfeed(enc=fake, Te=8, cf=fake, rs=None, fi=None, H=640, J=640, V=28, S=16, K=4, N=100, dt=0, ws=fake, opts=o):
        return lib.compute_rnnt_beam_stream_timed_feed(enc, Te, cf, rs, fi, H, J, V, S, K, N, dt, ws, opts)

    def sstep(pp=fake, par=fake, em=fake, tl=None, ts=None, lse=None, J=640, V=28, S=16, K=4, N=100, dt=0, ws=fake, opts=o):
        return lib.compute_rnnt_beam_stream_timed_step(pp, par, em, tl, ts, lse, J, V, S, K, N, dt, ws, opts)

    def sres(h=fake, n_=fake, sc=fake, stb=None, hf=fake, hl=fake, tst=None, J=640, V=28, S=16, K=4, N=100, dt=0, ws=fake, opts=o):
        return lib.compute_rnnt_beam_stream_timed_results(h, n_, sc, stb, hf, hl, tst, J, V, S, K, N, dt, ws, opts)

    calls = (gstep, gfeed, bbegin, bstep, bres, sbegin, sfeed, sstep, sres)
    cpu = _lib.make_options(0, 0, 8, 1, loc=_lib.RNNT_CPU)
    for call in calls:
        assert call(opts=cpu) == 2                              # device-only library
        assert call(opts=_lib.make_options(0, 28, 8, 1)) == 2   # blank_label >= alphabet_size
        assert call(opts=_lib.make_options(0, 0, 0, 1)) == 2    # maxT = 0
        assert call(ws=None) == 2 and call(ws=ctypes.c_void_p(256 + 64)) == 2  # workspace NULL / not 256-byte aligned
        assert call(dt=0x100) == 2 and call(dt=3) == 2          # no flag bits
        assert call(J=96) == 2 and call(V=4096) == 2 and call(V=0) == 2
    for call in (bbegin, bstep, bres, sbegin, sfeed, sstep, sres):
        assert call(K=0) == 2 and call(K=17) == 2
    for call in (sbegin, sfeed, sstep, sres):
        assert call(S=65, K=16) == 2 and call(S=0) == 2 and call(N=0) == 2 and call(S=64, K=16, N=big) == 2
    for k in ("pp", "h", "hf", "hl", "n_", "sc", "em", "ad"):
        assert gstep(**{k: None}) == 2, k
    for k in ("h", "hf", "hl", "fb"):
        assert gstep(**{k: odd}) == 2, k
    assert gstep(N=0) == 2 and gstep(B=0) == 2
    for k in ("cf", "n_", "sc", "ad", "fb"):
        assert gfeed(**{k: None}) == 2, k
    assert gfeed(fb=odd) == 2 and gfeed(Te=9) == 2 and gfeed(Te=-1) == 2 and gfeed(enc=None) == 2 and gfeed(H=0) == 2
    for k in ("ep", "fl", "w2", "b2"):
        assert bbegin(**{k: None}) == 2 and bbegin(**{k: odd}) == 2, k
    for k in ("pp", "par", "em"):
        assert bstep(**{k: None}) == 2 and sstep(**{k: None}) == 2, k
    for k in ("pp", "par", "em", "tl", "ts", "lse"):
        assert bstep(**{k: odd}) == 2 and sstep(**{k: odd}) == 2, k
    for k in ("h", "n_", "sc", "hf", "hl"):
        assert bres(**{k: None}) == 2 and bres(**{k: odd}) == 2 and sres(**{k: None}) == 2 and sres(**{k: odd}) == 2, k
    assert sres(stb=odd) == 2 and sres(tst=odd) == 2
    for k in ("w1", "b1", "w2", "b2"):
        assert sbegin(**{k: None}) == 2 and sbegin(**{k: odd}) == 2, k
    assert sbegin(H=0) == 2 and sbegin(H=4097) == 2
    assert sfeed(Te=9) == 2 and sfeed(enc=None) == 2 and sfeed(cf=None) == 2
    for k in ("enc", "cf", "rs", "fi"):
        assert sfeed(**{k: odd}) == 2, k
