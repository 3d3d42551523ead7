"""Per-token emission frames and log-probabilities on an MI355X, through compute_rnnt_greedy_step_timed,
compute_rnnt_greedy_stream_feed_timed and compute_rnnt_beam_[stream_]timed_*: the scripted scenarios against the float64
restatements of tests/token_time_cases.py (frames exactly, log-probabilities within one decision's score bar), every timed call
bitwise equal to its untimed twin in ids, lengths and scores, on 0xFF-filled workspaces and outputs too; greedy's (ids, frames)
re-scored on the materialised lattice and held against forced alignment; chunked streams in slot k of 16 bitwise equal to one
call, with a reset and a paused greedy stream; finality of what lies below the timed stable length; no scratch in the timed
kernels.  (The decoders have no HIP-graph replay test to mirror.)"""
import math

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib, alignment, decoding, joint as jmod
from rnnt_speech_recognition_amd.decoding import StreamingBeamDecoder, StreamingGreedyDecoder
from tests import decode_scripts as ds
from tests import test_greedy_batch_gpu as greedy_gpu
from tests import test_streaming_beam as cpu
from tests import token_time_cases as tt
from tests.test_decode_scripts_gpu import AbiBeam, AbiGreedy, LogitsEntry, _dev, _opts
from tests.test_frontend import small_model
from tests.test_isa_audit import _find, kernels  # noqa: F401  (module-scoped fixture: the built code objects)
from tests.test_streaming_beam_gpu import STREAM_SEEDS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


class TimedAbiBeam(AbiBeam):
    def __init__(self, sc, poison=False):
        super().__init__(sc, poison)
        self.ws = torch.zeros(_lib.beam_timed_workspace_bytes(sc.maxT, sc.B, sc.K, self.J, self.V, self.dtype), dtype=torch.uint8,
                              device=DEV)
        self.poison = poison
        if poison:
            self.ws.fill_(0xFF)

    def begin(self):
        sc = self.sc
        _lib.check(self.lib.compute_rnnt_beam_timed_begin(self.enc.data_ptr(), self.frames.data_ptr(), self.W2.data_ptr(),
                                                          self.b2.data_ptr(), self.J, self.V, sc.B, sc.K, self.dtype, self.ws.data_ptr(),
                                                          _opts(sc.blank, sc.maxT)), "compute_rnnt_beam_timed_begin")

    def step(self, rows):
        sc = self.sc
        self.rows.copy_(torch.from_numpy(rows))
        _lib.check(self.lib.compute_rnnt_beam_timed_step(self.rows.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(), None,
                                                         None, None, self.J, self.V, sc.B, sc.K, self.dtype, self.ws.data_ptr(),
                                                         _opts(sc.blank, sc.maxT)), "compute_rnnt_beam_timed_step")
        return self.parents.cpu().numpy(), self.emitted.cpu().numpy()

    def results(self):
        sc = self.sc
        fill = 0xFF if self.poison else 0
        hyps = torch.full((sc.B, sc.K, sc.maxT), -7, dtype=torch.int32, device=DEV)
        lengths = torch.full((sc.B, sc.K), -7, dtype=torch.int32, device=DEV)
        scores = torch.full((sc.B, sc.K), float("nan"), device=DEV)
        frames = torch.empty(sc.B, sc.K, sc.maxT, dtype=torch.int32, device=DEV)
        logp = torch.empty(sc.B, sc.K, sc.maxT, dtype=torch.float32, device=DEV)
        frames.view(torch.uint8).fill_(fill), logp.view(torch.uint8).fill_(fill)
        _lib.check(self.lib.compute_rnnt_beam_timed_results(hyps.data_ptr(), lengths.data_ptr(), scores.data_ptr(), frames.data_ptr(),
                                                            logp.data_ptr(), self.J, self.V, sc.B, sc.K, self.dtype, self.ws.data_ptr(),
                                                            _opts(sc.blank, sc.maxT)), "compute_rnnt_beam_timed_results")
        self.t_frames, self.t_logp = frames.cpu().numpy(), logp.cpu().numpy()
        return hyps.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy()


class TimedAbiGreedy(AbiGreedy):
    """hyp_frames / hyp_logp start as -1 / 0 (append-only outputs: the library writes a token's place and nothing else)."""

    def begin(self, max_hyp_len):
        super().begin(max_hyp_len)
        self.f = torch.full((self.sc.B, max_hyp_len), -1, dtype=torch.int32, device=DEV)
        self.l = torch.zeros(self.sc.B, max_hyp_len, device=DEV)

    def step(self, rows):
        sc = self.sc
        self.rows.copy_(torch.from_numpy(rows))
        _lib.check(self.lib.compute_rnnt_greedy_step_timed(self.rows.data_ptr(), self.h.data_ptr(), self.f.data_ptr(), self.l.data_ptr(),
                                                           self.h.shape[1], self.lengths.data_ptr(), self.scores.data_ptr(),
                                                           self.emitted.data_ptr(), self.all_done.data_ptr(), None, None, self.J, self.V,
                                                           sc.B, self.dtype, self.ws.data_ptr(), _opts(sc.blank, sc.maxT)),
                   "compute_rnnt_greedy_step_timed")
        return self.emitted.cpu().numpy(), int(self.all_done.cpu()[0]), self.lengths.cpu().numpy(), self.scores.cpu().numpy()

    def grow(self, max_hyp_len):
        n = self.h.shape[1]
        super().grow(max_hyp_len)
        f = torch.full((self.sc.B, max_hyp_len), -1, dtype=torch.int32, device=DEV)
        l = torch.zeros(self.sc.B, max_hyp_len, device=DEV)
        f[:, :n], l[:, :n] = self.f, self.l
        self.f, self.l = f, l


def _beam(sc):
    fn = LogitsEntry(sc)
    args = (sc.joint, sc.script, sc.B, sc.K, sc.frames, sc.maxT, sc.blank, sc.steps, fn, sc.ties_allowed)
    eng = TimedAbiBeam(sc)
    trace, ref, _, _ = ds.run_beam(eng, *args)
    plain = ds.run_beam(AbiBeam(sc), *args, check=False)[0]
    assert ds.traces_equal(trace, plain), "the timed calls changed ids, lengths, scores, parents or emitted"
    want = tt.restate_beam(sc, fn)
    assert [[y for y, _ in b] for b in want.beams] == [[y for y, _ in b] for b in ref.beams]
    err, bar = tt.check_beam_times(sc, want, trace[-1][1], eng.t_frames, eng.t_logp)
    print(f"[{sc.name}] frames exact; worst log-probability error {err:.3e} (bar {bar:.3e})")
    bad = TimedAbiBeam(sc, poison=True)
    poisoned = ds.run_beam(bad, *args, check=False)[0]
    assert ds.traces_equal(trace, poisoned) and np.array_equal(bad.t_frames, eng.t_frames)
    assert bad.t_logp.tobytes() == eng.t_logp.tobytes(), "0xFF-filled workspace and outputs changed the times"
    return eng, want


def _greedy(sc):
    fn = LogitsEntry(sc)
    args = (sc.joint, sc.script, sc.B, sc.frames, sc.max_symbols, sc.max_per_frame, sc.maxT, sc.blank, sc.hyp_lens, fn,
            sc.ties_allowed)
    eng = TimedAbiGreedy(sc)
    trace, ref, _, _ = ds.run_greedy(eng, *args)
    plain = ds.run_greedy(AbiGreedy(sc), *args, check=False)[0]
    assert ds.traces_equal(trace, plain), "the timed step changed ids, lengths, scores, emitted or all_done"
    want = tt.restate_greedy(sc, fn)
    assert want.y == ref.y
    frames, logp = eng.f.cpu().numpy(), eng.l.cpu().numpy()
    err, bar = tt.check_greedy_times(sc, want, frames, logp)
    print(f"[{sc.name}] frames exact; worst log-probability error {err:.3e} (bar {bar:.3e})")
    bad = TimedAbiGreedy(sc, poison=True)
    poisoned = ds.run_greedy(bad, *args, check=False)[0]
    assert ds.traces_equal(trace, poisoned) and np.array_equal(bad.f.cpu().numpy(), frames)
    assert bad.l.cpu().numpy().tobytes() == logp.tobytes(), "a 0xFF-filled workspace changed the times"
    return eng, want


# ---- scripted scenarios through the C ABI --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 5, 8, 16])
def test_forced_merges_keep_the_survivors_frames(K):
    _, want = _beam(ds.merge_scenario(K))
    assert want.ev.merges >= 4


def test_the_first_ranked_member_of_a_merge_keeps_its_frame():
    sc = tt.late_twin_scenario()
    sc.steps = 2
    eng, want = _beam(sc)
    assert want.ev.merges == 1 and [y for y, _ in want.beams[0]][:2] == [(1,), (1, 2)]
    assert eng.t_frames[0, 0, 0] == 1 and eng.t_frames[0, 1, :2].tolist() == [0, 1]
    _beam(tt.late_twin_scenario())


@pytest.mark.parametrize("K", [1, 2, 5, 16])
def test_exact_ties(K):
    _beam(ds.tie_scenario(K))


def test_random_script_full_beam_and_nothing_taken():
    _beam(ds.small_vocabulary_scenario())
    _beam(ds.full_beam_scenario())
    _beam(ds.nothing_taken_scenario())


@pytest.mark.parametrize("cap", [0, 1, 2, 3])
def test_greedy_symbol_caps(cap):
    _greedy(ds.greedy_caps_scenario(cap))


def test_greedy_batch_beyond_one_pass():
    _greedy(ds.greedy_batch_scenario(257))


def test_greedy_pause_and_resume_carries_frames_and_logp():
    small, _ = _greedy(ds.greedy_pause_scenario([3, 5, 40]))
    large, _ = _greedy(ds.greedy_pause_scenario([40]))
    assert torch.equal(small.f, large.f) and torch.equal(small.l.view(torch.int32), large.l.view(torch.int32))


@pytest.mark.parametrize("dtype", [0, 1])
def test_greedy_exact_argmax_ties_pin_the_frames(dtype):
    eng, want = _greedy(ds.greedy_tie_scenario(dtype))
    assert want.ev.ties >= 8 and eng.f[0, :8].tolist() == [0, 0, 2, 2, 3, 3, 4, 4]


# ---- a real Transducer: the untimed twin ---------------------------------------------------------------------------------------
def _model(vocab):
    if vocab in (12, 4096):
        return greedy_gpu._decode_model(vocab)
    model = small_model(3, vocab_size=vocab)
    with torch.no_grad():
        model.joint.b2[0] -= 0.4
    return model.to(DEV).eval()


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


@pytest.mark.parametrize("vocab", [28, 4096])
def test_timed_decodes_of_a_transducer_are_bitwise_the_untimed_ones(vocab):
    model = _model(vocab)
    torch.manual_seed(18)
    mel = torch.randn(8, 30, 8).to(DEV)
    spec_lengths = torch.tensor([30, 25, 30, 4, 17, 30, 9, 21], device=DEV)
    for prediction in ("torch", "engine"):
        plain = decoding.greedy_decode_batch(model, mel, spec_lengths, max_length=40, prediction=prediction)
        timed = decoding.greedy_decode_batch(model, mel, spec_lengths, max_length=40, prediction=prediction, token_times=True)
        assert jmod.GreedyJoint(model.joint).engine and len(timed) == 5 and int(timed[1].sum()) >= 8
        for a, b in zip(plain, timed):
            assert torch.equal(_bits(a), _bits(b)), (vocab, prediction, "greedy")
        ids, n, _, frames, logp = timed
        live = torch.arange(ids.shape[1], device=DEV)[None, :] < n[:, None]
        assert (frames[live] >= 0).all() and (frames[~live] == -1).all() and not logp[~live].any() and (logp[live] <= 0).all()
        assert (frames[:, 1:][live[:, 1:]] >= frames[:, :-1][live[:, 1:]]).all()  # a frame cursor never goes back
        for K in (1, 4):
            plain = decoding.beam_decode_batch(model, mel, spec_lengths, beam=K, prediction=prediction)
            timed = decoding.beam_decode_batch(model, mel, spec_lengths, beam=K, prediction=prediction, token_times=True)
            for a, b in zip(plain, timed):
                assert torch.equal(_bits(a), _bits(b)), (vocab, prediction, "beam", K)
            ids, n, _, frames, logp = timed
            live = torch.arange(ids.shape[1], device=DEV)[None, :] < n[:, None]
            assert (frames[live] >= 0).all() and (frames[~live] == -1).all() and not logp[~live].any()
            assert (frames[:, 1:][live[:, 1:]] > frames[:, :-1][live[:, 1:]]).all()  # one symbol per frame


# ---- consistency with the lattice ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [12, 28])
def test_greedy_times_describe_a_path_of_the_lattice(vocab):
    # (seed and blank bias picked on the torch route: some utterances run out of frames with tokens spread over several of them,
    # others repeat a symbol until the budget is spent)
    model = small_model(7 if vocab == 12 else 5, vocab_size=vocab)
    with torch.no_grad():
        model.joint.b2[0] += 0.6 if vocab == 12 else 1.0
    model = model.to(DEV).eval()
    torch.manual_seed(18)
    mel = torch.randn(8, 30, 8).to(DEV)
    spec_lengths = torch.tensor([30, 25, 30, 4, 17, 30, 9, 21], device=DEV)
    budget = 40  # (no per-frame cap: a forced frame advance is no move of the lattice)
    ids, n, scores, frames, logp = decoding.greedy_decode_batch(model, mel, spec_lengths, max_length=budget, token_times=True)
    with torch.no_grad():
        enc = model.encoder(mel)
        U = int(n.max()) + 1
        pred_in = torch.nn.functional.pad(ids[:, : U - 1].long(), (1, 0))  # the start token 0, then the hypothesis
        pred = model.prediction(pred_in)
        jn = model.joint
        acts = jmod.joint_logits(enc, pred, jn.W1.detach(), jn.b1.detach(), jn.W2.detach(), jn.b2.detach()).float().contiguous()
    T = pkg.reduced_lengths(spec_lengths, model.hp.time_reduction_factor)
    lp = torch.log_softmax(acts.double(), dim=-1).cpu()
    max_lse = float(torch.logsumexp(acts.double(), dim=-1).abs().max())
    worst_tok, worst_path = (0.0, 0.0), (0.0, 0.0)
    ends, closing = [], []  # per utterance: the frames its path covers, and the blank that closes it where greedy left it open
    for b in range(8):
        nb, Tb = int(n[b]), int(T[b])
        fr, total, u, steps = frames[b, :nb].tolist(), 0.0, 0, 0
        for t in range(Tb):  # the path: every label recorded at t, then the blank that leaves the frame
            while u < nb and fr[u] == t:
                cell = float(lp[b, t, u, int(ids[b, u])])
                err, bar = abs(float(logp[b, u]) - cell), ds.score_bar(1, max_lse, cell)
                worst_tok = max(worst_tok, (err, bar))
                assert err <= bar, (b, u, float(logp[b, u]), cell, err, bar)
                total, u, steps = total + cell, u + 1, steps + 1
            if u < budget:  # (a hypothesis that spent its symbol budget stops inside the frame)
                total, steps = total + float(lp[b, t, u, 0]), steps + 1
        assert u == nb
        if nb < budget:  # out of frames: a whole path of the lattice, its last blank included
            ends.append(Tb), closing.append(0.0)
        else:  # out of symbols inside frame fr[-1]: the blank of that cell would end a lattice of fr[-1] + 1 frames
            ends.append(fr[-1] + 1), closing.append(float(lp[b, fr[-1], nb, 0]))
        err, bar = abs(float(scores[b]) - total), ds.score_bar(steps, max_lse, total)
        worst_path = max(worst_path, (err, bar))
        assert err <= bar, (b, float(scores[b]), total, err, bar)
    print(f"[lattice V={vocab}] token log-probability error {worst_tok[0]:.3e} (bar {worst_tok[1]:.3e}); "
          f"path score error {worst_path[0]:.3e} (bar {worst_path[1]:.3e})")
    # forced alignment of the greedy ids finds a path at least as good as the one greedy took.  An untrained model repeats a
    # symbol until its budget is spent, so most utterances stop inside a frame: their path plus that cell's blank is a whole
    # path of the lattice cut after that frame, and the alignment runs over exactly those frames.
    _, _, best = alignment.rnnt_align(acts, ids[:, : U - 1], torch.tensor(ends, dtype=torch.int32, device=DEV), n, blank_label=0)
    best, took = best.cpu().double(), scores.cpu().double() + torch.tensor(closing, dtype=torch.float64)
    spread = [b for b in range(8) if 2 <= int(n[b]) < budget and int(frames[b, int(n[b]) - 1]) >= 1]
    assert spread, ("precondition: no utterance ends by frames with tokens beyond frame 0", n.tolist())
    print(f"[lattice V={vocab}] tokens {n.tolist()}, frames covered {ends} of {T.tolist()}; best path - greedy path: "
          f"{[round(float(x), 6) for x in best - took]}")
    assert (best >= took - 1e-4 * took.abs().clamp(min=1.0)).all(), (best, took)


# ---- streams -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [12, 4096])
def test_chunked_greedy_streams_are_bitwise_one_call_times_included(vocab):
    model = _model(vocab)
    f = model.encoder.reduce.factor
    X = cpu.seeded_streams(model, cpu.LENGTHS, STREAM_SEEDS[vocab], DEV)

    def one(x, N):
        dec = StreamingGreedyDecoder(model, 1, x.shape[0], max_length=N, token_times=True)
        assert dec.gj.engine
        dec.start([0])
        dec.feed(x[None], [x.shape[0]], [True])
        return tt.read_timed_greedy(dec, 0)

    want = [one(x, 40) for x in X]
    assert sum(len(w[0]) for w in want) >= 8
    untimed = StreamingGreedyDecoder(model, 1, X[0].shape[0], max_length=40)
    untimed.start([0])
    untimed.feed(X[0][None], [X[0].shape[0]], [True])
    hi, hl, hs = untimed.hypotheses()
    assert hi[0, : int(hl[0])].tolist() == want[0][0] and hs[0].cpu().numpy().tobytes() == want[0][3]
    for kind in ["f", "random"]:
        plans, Tc = cpu.plans_for(cpu.LENGTHS, f, kind, 5, cpu.SLOTS)
        dec = StreamingGreedyDecoder(model, 16, Tc, max_length=40, check_every=3, token_times=True)
        got = tt.run_streams(dec, X, plans, tt.read_timed_greedy, seed=len(kind), extra_restart=(2, 11))
        for i, w in enumerate(want):
            assert got[i] == w, (kind, i, got[i][:2], w[:2])
    # a slot that is started again restarts at frame 0 (slot 1 of 2 decodes stream 0, then stream 1)
    dec = StreamingGreedyDecoder(model, 2, 32, max_length=40, token_times=True)
    for i in (0, 1):
        dec.start([1])
        mel = torch.zeros(2, 32, X[i].shape[1], device=DEV)
        mel[1, : X[i].shape[0]] = X[i]
        dec.feed(mel, [0, X[i].shape[0]], [False, True])
        assert tt.read_timed_greedy(dec, 1) == want[i], i
    # no symbol budget: the hyps buffer (encoder frames + 16) fills, the stream pauses, all three buffers grow, it resumes
    with torch.no_grad():
        model.joint.b2[0] -= 30.0  # (symbols at every decision until the per-frame cap)
    x = X[0]
    plans, Tc = cpu.plans_for(cpu.LENGTHS[:1], f, "f", 5, [3])
    dec = StreamingGreedyDecoder(model, 4, Tc, max_symbols_per_frame=6, check_every=1, token_times=True)
    n0 = dec.gj.hyps.shape[1]
    got = tt.run_streams(dec, [x], plans, tt.read_timed_greedy)
    assert dec.gj.hyps.shape[1] > n0 and dec.gj.frames.shape == dec.gj.hyps.shape == dec.gj.logp.shape, "the stream never paused"
    big = StreamingGreedyDecoder(model, 1, x.shape[0], max_length=10000, max_symbols_per_frame=6, token_times=True)
    big.start([0])
    big.feed(x[None], [x.shape[0]], [True])
    assert got[0] == tt.read_timed_greedy(big, 0) and len(got[0][0]) > n0  # (ids, frames, logp bits, score bits)


@pytest.mark.parametrize("vocab", [12, 4096])
@pytest.mark.parametrize("K", [1, 4, 8])
def test_chunked_beam_streams_are_bitwise_one_call_times_included(vocab, K):
    model = _model(vocab)
    f = model.encoder.reduce.factor
    X = cpu.seeded_streams(model, cpu.LENGTHS, STREAM_SEEDS[vocab], DEV)
    N = 24

    def one(x):
        dec = StreamingBeamDecoder(model, 1, x.shape[0], beam=K, max_length=N, token_times=True)
        assert dec.bj.engine
        dec.start([0])
        dec.feed(x[None], [x.shape[0]], [True])
        return tt.read_timed_beam(dec, 0)

    want = [one(x) for x in X]
    assert sum(len(w[0][0][0]) for w in want) >= 8
    plain = cpu.one_call(model, X[0], K, N)  # the untimed twin: ids and scores bitwise
    assert plain[0] == [r[0] for r in want[0][0]] and plain[3] == want[0][1]
    assert plain[2][: len(plain[0])].cpu().numpy().tobytes() == b"".join(r[3] for r in want[0][0])
    final = {}

    def finality(dec, owner):  # the (token, frame) pairs below the timed stable length are reported unchanged ever after
        ids, _, _, frames, _ = dec.timed_nbest()
        tst, st = dec.timed_stable_lengths().tolist(), dec.bj.results()[3].tolist()
        for slot, i in owner.items():
            assert tst[slot] <= st[slot]
            pairs = list(zip(ids[slot, 0, : tst[slot]].tolist(), frames[slot, 0, : tst[slot]].tolist()))
            old = final.get(i, [])
            assert pairs[: len(old)] == old, (i, old, pairs)
            final[i] = pairs if len(pairs) > len(old) else old

    for kind in ["f", "random"]:
        final.clear()
        plans, Tc = cpu.plans_for(cpu.LENGTHS, f, kind, 5, cpu.SLOTS)
        dec = StreamingBeamDecoder(model, 16, Tc, beam=K, max_length=N, token_times=True)
        got = tt.run_streams(dec, X, plans, tt.read_timed_beam, seed=len(kind), extra_restart=(2, 11), after_feed=finality)
        for i, w in enumerate(want):
            assert got[i] == w, (kind, i)


class _ScriptedStream:
    """compute_rnnt_beam_stream_timed_* fed with a scripted scenario, `chunk` frames per feed, one slot."""

    def __init__(self, sc, chunk):
        sj = sc.joint
        self.sc, self.J, self.V, self.dtype, self.chunk = sc, sj.J, sj.V, sj.dtype, chunk
        W2, b2 = sj.weights()
        self.W2, self.b2 = _dev(W2), _dev(b2)
        self.W1, self.b1 = torch.zeros(1, self.J, device=DEV), torch.zeros(self.J, device=DEV)
        self.N = sc.maxT
        self.ws = torch.empty(_lib.beam_stream_timed_workspace_bytes(chunk, 1, sc.K, self.N, 1, self.J, self.V, self.dtype),
                              dtype=torch.uint8, device=DEV).fill_(0xFF)
        self.parents = torch.zeros(sc.K, dtype=torch.int32, device=DEV)
        self.emitted = torch.zeros(sc.K, dtype=torch.int32, device=DEV)
        self.rows = torch.empty(sc.K, self.J, device=DEV)
        self.lib, self.o = _lib.load(), _opts(sc.blank, chunk)
        self.args = (self.J, self.V, 1, sc.K, self.N, self.dtype, self.ws.data_ptr(), self.o)
        _lib.check(self.lib.compute_rnnt_beam_stream_timed_begin(self.W1.data_ptr(), self.b1.data_ptr(), self.W2.data_ptr(),
                                                                 self.b2.data_ptr(), 1, *self.args), "begin")

    def feed(self, reset, final):
        enc = torch.zeros(1, self.chunk, 1, device=DEV)
        v = lambda x: torch.tensor([x], dtype=torch.int32, device=DEV)  # noqa: E731
        self.keep = (enc, v(self.chunk), v(int(reset)), v(int(final)))
        _lib.check(self.lib.compute_rnnt_beam_stream_timed_feed(enc.data_ptr(), self.chunk, *(x.data_ptr() for x in self.keep[1:]), 1,
                                                                *self.args), "feed")

    def step(self, rows):
        self.rows.copy_(torch.from_numpy(rows))
        _lib.check(self.lib.compute_rnnt_beam_stream_timed_step(self.rows.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(),
                                                                None, None, None, *self.args), "step")
        return self.parents.cpu().tolist(), self.emitted.cpu().tolist()

    def results(self):
        K, N = self.sc.K, self.N
        out = [torch.empty(1, K, N, dtype=torch.int32, device=DEV), torch.empty(1, K, dtype=torch.int32, device=DEV),
               torch.empty(1, K, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV),
               torch.empty(1, K, N, dtype=torch.int32, device=DEV), torch.empty(1, K, N, device=DEV),
               torch.empty(1, dtype=torch.int32, device=DEV)]
        _lib.check(self.lib.compute_rnnt_beam_stream_timed_results(*(x.data_ptr() for x in out), *self.args), "results")
        return [x.cpu().numpy() for x in out]


def test_finality_when_hypotheses_share_tokens_but_not_frames():
    sc = tt.late_twin_scenario()
    fn = LogitsEntry(sc)
    ref = tt.TimedBeamRestatement(fn, sc.B, sc.K, sc.frames, sc.maxT, sc.blank)
    eng = _ScriptedStream(sc, chunk=1)  # one frame per feed: results after every frame
    seqs, seen, final = [()] * sc.K, [], []
    for t in range(sc.steps):
        eng.feed(reset=t == 0, final=t == sc.steps - 1)
        L = np.stack([sc.script(0, t, seqs[k]) if k < len(ref.beams[0]) else np.full(sc.V, -0.37 * 16.0) for k in range(sc.K)])
        parents, emitted = eng.step(sc.joint.pred_rows(L))
        want_p, want_e = ref.step()
        assert parents == want_p and emitted == want_e, t
        seqs = [seqs[p] + ((e,) if e >= 0 else ()) for p, e in zip(parents, emitted)]
        hyps, lengths, _, stable, frames, logp, tstable = eng.results()
        toks = [list(y) for y, _ in ref.beams[0]]
        assert int(stable[0]) == cpu.common_prefix(toks) and int(tstable[0]) == ref.timed_stable(0) <= int(stable[0]), t
        for k, row in enumerate(ref.times[0]):
            tt.check_row(frames[0, k], logp[0, k], row, ref.ev.max_lse, (t, k))
        pairs = list(zip(hyps[0, 0, : int(tstable[0])].tolist(), frames[0, 0, : int(tstable[0])].tolist()))
        assert pairs[: len(final)] == final, (t, final, pairs)
        final = pairs if len(pairs) > len(final) else final
        seen.append((int(stable[0]), int(tstable[0])))
    assert any(ts < s for s, ts in seen) and seen[-1][1] >= 1, seen  # (the script does what it was written for)
    print(f"[late-twin] (stable, timed stable) per frame: {seen}")


# ---- the code objects ----------------------------------------------------------------------------------------------------------
def test_timed_kernels_use_no_scratch(kernels):  # noqa: F811
    meta, _ = kernels
    names = [k for k in meta if any(s in k for s in ("greedy_update_timed_kernel", "greedy_stream_feed_timed_kernel",
                                                     "beam_select_timed_kernel", "beam_results_timed_kernel"))]
    assert len(names) == 4, names
    for k in names:
        assert int(meta[k]["private_segment_fixed_size"]) == 0 and int(meta[k].get("vgpr_spill_count", "0")) == 0, (k, meta[k])
