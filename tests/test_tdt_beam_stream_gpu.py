"""Streaming TDT beam search on an MI355X, through the C ABI (compute_rnnt_tdt_beam_stream_*) and through tdt.TDTBeamStreamJoint /
tdt.StreamingTDTBeamDecoder.  The scenarios of tests/tdt_beam_stream_cases.py run against the float64 restatement of each stream's
whole utterance, fed with the f32 logits compute_rnnt_joint_logits returns for each hypothesis alone: parents, emitted, ids, lengths,
cursors, frames, durations and both stable lengths exactly at every step; scores within tdt_beam_cases.score_bar, the bar of
tests/test_tdt_beam_gpu.py (the library reports f32 scores).  Every equivalence the header states is checked BIT FOR BIT: a chunking
against the single chunk, a slot against slot 0 of a 1-slot decoder, the single chunk against the offline compute_rnnt_tdt_beam_*."""
import numpy as np
import pytest
import torch

from rnnt_speech_recognition_amd import _lib, tdt
from rnnt_speech_recognition_amd import joint as jmod
from rnnt_speech_recognition_amd.decoding import StreamingTranscriber
from tests import frontend_cases as fc
from tests import tdt_beam_cases as bc
from tests import tdt_beam_stream_cases as sc_
from tests.test_tdt_beam_gpu import AbiBeam
from tests.test_tdt_greedy_gpu import LogitsEntry, _dev, _opts
from tests.test_tdt_stream import DUR, small_tdt_stream_model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


class AbiStream:
    """The caller of the C ABI.  poison: the workspace holds 0xFF bytes (NaN) on entry; diag: the token diagnostics."""

    def __init__(self, sc, timed=True, diag=True, poison=True):
        c = self.case = sc.case
        self.sc, self.timed = sc, timed
        self.W1, self.b1 = torch.zeros(sc_.H, c.J, device=DEV), torch.zeros(c.J, device=DEV)
        self.W2, self.b2 = _dev(c.W2), _dev(c.b2)
        nbytes = _lib.tdt_beam_stream_workspace_bytes(sc.Tc, sc.S, sc.K, sc.N, sc_.H, c.J, c.V, c.D, c.dtype, timed)
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        assert self.ws.data_ptr() % 256 == 0
        if poison:
            self.ws.fill_(0xFF)
        R = sc.S * sc.K
        self.parents = torch.full((R,), -7, dtype=torch.int32, device=DEV)
        self.emitted = torch.full((R,), -7, dtype=torch.int32, device=DEV)
        self.rows = torch.empty(R, c.J, device=DEV)
        self.tops_dev = torch.full((R, sc.K), -7, dtype=torch.int32, device=DEV) if diag else None
        self.tops = None
        self.dur = (_lib.ctypes.c_int * c.D)(*c.durations)
        self.lib = _lib.load_tdtbeamstream()

    def _tail(self):
        c, sc = self.case, self.sc
        return (c.J, c.V, c.D, sc.S, sc.K, sc.N, c.dtype, int(self.timed), self.ws.data_ptr(), _opts(c.blank, sc.Tc))

    def begin(self):
        c = self.case
        torch.cuda.synchronize()
        _lib.check(self.lib.compute_rnnt_tdt_beam_stream_begin(self.W1.data_ptr(), self.b1.data_ptr(), self.W2.data_ptr(), self.b2.data_ptr(),
                                                               sc_.H, c.J, c.V, self.dur, *self._tail()[2:]), "begin")

    def feed(self, enc, frames, reset, final):
        Te = 0 if enc is None else enc.shape[1]
        self.keep = (None if enc is None else _dev(enc), _dev(np.asarray(frames, np.int32)), _dev(np.asarray(reset, np.int32)),
                     _dev(np.asarray(final, np.int32)))
        e, fr, rs, fi = self.keep
        torch.cuda.synchronize()
        _lib.check(self.lib.compute_rnnt_tdt_beam_stream_feed(None if e is None else e.data_ptr(), Te, fr.data_ptr(), rs.data_ptr(),
                                                              fi.data_ptr(), sc_.H, *self._tail()), "feed")

    def step(self, rows):
        self.rows.copy_(torch.from_numpy(rows))
        if self.tops_dev is not None:
            self.tops_dev.fill_(-7)
        torch.cuda.synchronize()
        _lib.check(self.lib.compute_rnnt_tdt_beam_stream_step(self.rows.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(), None,
                                                              None if self.tops_dev is None else self.tops_dev.data_ptr(), None, None,
                                                              *self._tail()), "step")
        torch.cuda.synchronize()
        self.tops = None if self.tops_dev is None else self.tops_dev.cpu().numpy()
        return self.parents.cpu().numpy(), self.emitted.cpu().numpy()

    def results(self):
        sc = self.sc
        S, K, N = sc.S, sc.K, sc.N
        i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=DEV)  # noqa: E731
        hyps, lengths, cursors, stable = i32(S, K, N), i32(S, K), i32(S, K), i32(S)
        scores = torch.full((S, K), float("nan"), device=DEV)
        fr, du, ts = (i32(S, K, N), i32(S, K, N), i32(S)) if self.timed else (None, None, None)
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        torch.cuda.synchronize()
        _lib.check(self.lib.compute_rnnt_tdt_beam_stream_results(hyps.data_ptr(), lengths.data_ptr(), scores.data_ptr(), cursors.data_ptr(),
                                                                 stable.data_ptr(), ptr(fr), ptr(du), ptr(ts), *self._tail()), "results")
        torch.cuda.synchronize()
        return tuple(None if x is None else x.cpu().numpy() for x in (hyps, lengths, scores, stable, cursors, fr, du, ts))


class PyStream:
    """The same caller through tdt.TDTBeamStreamJoint (the engine route)."""

    def __init__(self, sc):
        c = sc.case
        joint = type("J", (), dict(W1=torch.zeros(sc_.H, c.J, device=DEV), b1=torch.zeros(c.J, device=DEV), W2=_dev(c.W2), b2=_dev(c.b2),
                                   blank_label=c.blank))
        self.sc, self.tops = sc, None
        self.jb = tdt.TDTBeamStreamJoint(joint, c.durations, sc.K, joint_dtype=("f32", "f16")[c.dtype], token_times=True)
        assert self.jb.engine and self.jb.Jp == c.J

    def begin(self):
        self.jb.begin(self.sc.S, self.sc.Tc, self.sc.N)
        assert self.jb.engine

    def feed(self, enc, frames, reset, final):
        self.jb.feed(None if enc is None else _dev(enc), frames, reset, final)

    def step(self, rows):
        parents, emitted = self.jb.step(pred_proj=_dev(rows))
        return parents.cpu().numpy(), emitted.cpu().numpy()

    def results(self):
        return tuple(x.cpu().numpy() for x in self.jb.results())


def bar(got, want, steps, ref):
    return abs(got - want) <= bc.score_bar(max(steps, 1), ref.ev.max_lse, want)


def _run(sc, engine=None, **kw):
    return sc_.run_streams(engine or AbiStream(sc, **kw), sc, LogitsEntry(sc.case), bar)


_ONE = {}


def _one(dtype=0, K=4):
    """The single-chunk decode of the 13-frame stream in a 1-slot decoder: computed once, shared, left unchanged."""
    if (dtype, K) not in _ONE:
        _ONE[dtype, K] = _run(sc_.chunking_scenario("one", K=K, dtype=dtype)).results[0]
    return _ONE[dtype, K]


@pytest.mark.parametrize("dtype", [0, 1])
def test_single_chunk_is_the_offline_decoder_bit_for_bit(dtype):
    sc = sc_.chunking_scenario("one", dtype=dtype)
    off = bc.Scenario(sc.case.name, sc.case, sc.K, sc_.T13)
    trace, ref, _, _ = bc.run_tdt_beam(AbiBeam(off, poison=True), off, LogitsEntry(sc.case), every_step=False)
    hyps, lengths, scores, cursors, frames, durs = (x[0] for x in trace[-1])
    one = _one(dtype)
    assert sc_.same_bits((hyps, lengths, scores, cursors, frames, durs), (one[0], one[1], one[2], one[4], one[5], one[6]))
    assert ref.ev.merges >= 1 and lengths.max() >= 1


@pytest.mark.parametrize("name", [n for n in sc_.CHUNKINGS if n != "one"])
@pytest.mark.parametrize("dtype", [0, 1])
def test_every_chunking_gives_the_bits_of_the_single_chunk(name, dtype):
    out = _run(sc_.chunking_scenario(name, dtype=dtype))
    assert sc_.same_bits(out.results[0], _one(dtype))
    assert out.tops_checked == out.refs[0].ev.active_rows and out.steps == 13


def test_a_carry_that_outlives_several_feeds():
    one = _run(sc_.long_carry_scenario(14)).results[0]
    for chunk in (1, 2, 3):
        out = _run(sc_.long_carry_scenario(chunk))
        assert sc_.same_bits(out.results[0], one)
        ev = out.refs[0].ev
        assert ev.idle_full >= 4 and ev.past_end >= 1 and 8 in ev.durations_used


def test_merges_and_non_merges_across_a_boundary():
    one = _run(sc_.boundary_merge_scenario(9)).results[0]
    for chunk in (1, 2):
        out = _run(sc_.boundary_merge_scenario(chunk))
        assert sc_.same_bits(out.results[0], one)
        ev = out.refs[0].ev
        assert ev.stay_merges >= 1 and ev.kept_apart >= 1 and ev.aligned_later >= 1


@pytest.mark.parametrize("slot", [0, 2, 3])
def test_the_same_stream_in_any_slot_beside_other_traffic(slot):
    out = _run(sc_.slots_scenario(slot))
    assert sc_.same_bits(out.results[0], _one()) and out.frozen_steps > 0


def test_final_chunk_freezes_the_slot_until_a_reset():
    out = _run(sc_.final_scenario())
    assert sc_.same_bits(out.results[1], _one())
    cut = out.results[0]
    assert out.refs[0].t == 9 and (cut[4][cut[1] > 0] >= 9).all() and out.frozen_steps > 0


@pytest.mark.parametrize("N", [1, 2])
def test_a_full_hypothesis_offers_its_blank_alone(N):
    one = _run(sc_.n_rule_scenario(N, chunks=(10,)))
    ref = one.refs[0]
    assert ref.full_rows > 0 and ref.blank_outside > 0 and (N == 1 or ref.mixed_frames > 0) and one.tops_checked > 0
    assert (one.results[0][1] <= N).all() and (one.results[0][1] == N).any()
    for chunks in ((2, 1, 3, 4), (1,) * 10):
        assert sc_.same_bits(_run(sc_.n_rule_scenario(N, chunks=chunks)).results[0], one.results[0])


def test_a_row_of_nan_logits_carries_the_beam_over():
    out = _run(sc_.nan_scenario())
    assert out.refs[0].ev.carried == [(0, 4)] and out.refs[0].ev.dropped >= 1


GEOMETRY = {
    "beam-1": dict(S=3, K=1, slot=1),
    "beam-16": dict(S=2, K=16, slot=1),
    "33-rows": dict(S=11, K=3, slot=10),           # S K = 33: the stream's rows lie in the second 32-row tile
    "272-rows": dict(S=17, K=16, slot=16),         # beyond 256 rows
    "head-straddles": dict(S=2, K=4, slot=1, V=30, durations=[0, 1, 2, 3]),  # columns 30 ... 33: two 32-column chunks
    "two-slices-f16": dict(S=2, K=4, slot=1, V=130, durations=[0, 1, 2, 3], dtype=1, J=256),  # 134 columns: two slices
    "f16": dict(S=2, K=4, slot=0, dtype=1),
}


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_geometry(name):
    kw = dict(GEOMETRY[name])
    out = _run(sc_.geometry_scenario(**kw))
    kw.update(S=1, slot=0)
    one = _run(sc_.geometry_scenario(**kw))
    assert sc_.same_bits(out.results[0], one.results[0])


def test_untimed_two_runs_and_a_clean_workspace_give_the_same_bits():
    sc = sc_.chunking_scenario("cuts")
    a = _run(sc).results[0]
    assert sc_.same_bits(a, _run(sc).results[0])                    # two identical decodes
    assert sc_.same_bits(a, _run(sc, poison=False).results[0])      # a zeroed workspace against the NaN-poisoned one
    b = _run(sc, timed=False).results[0]
    assert sc_.same_bits(a[:5], b[:5]) and b[5] is None


def test_invalid_calls_enqueue_nothing():
    sc = sc_.chunking_scenario("one")
    eng = AbiStream(sc)
    eng.begin()
    eng.feed(np.zeros((1, 13, sc_.H), np.float32), [13], [1], [1])
    torch.cuda.synchronize()
    before = eng.ws.clone()
    c, lib = sc.case, eng.lib
    tail = eng._tail()
    rows = torch.zeros(sc.K, c.J, device=DEV)
    out = torch.full((sc.K,), -7, dtype=torch.int32, device=DEV)
    bad_opts = _opts(c.V, sc.Tc)  # the blank inside the duration head
    assert lib.compute_rnnt_tdt_beam_stream_step(rows.data_ptr(), out.data_ptr(), out.data_ptr(), None, None, None, None, *tail[:-1], bad_opts) == 2
    assert lib.compute_rnnt_tdt_beam_stream_step(rows.data_ptr(), out.data_ptr(), out.data_ptr(), None, None, None, None, c.J, c.V, c.D, sc.S,
                                                 17, *tail[5:]) == 2
    assert lib.compute_rnnt_tdt_beam_stream_feed(None, 14, out.data_ptr(), None, None, sc_.H, *tail) == 2
    assert lib.compute_rnnt_tdt_beam_stream_results(out.data_ptr(), out.data_ptr(), out.data_ptr(), None, None, out.data_ptr(), None, None,
                                                    *tail) == 2
    bad = (_lib.ctypes.c_int * c.D)(*([0] * c.D))
    assert lib.compute_rnnt_tdt_beam_stream_begin(eng.W1.data_ptr(), eng.b1.data_ptr(), eng.W2.data_ptr(), eng.b2.data_ptr(), sc_.H, c.J, c.V,
                                                  bad, *tail[2:]) == 2
    torch.cuda.synchronize()
    assert torch.equal(eng.ws, before) and (out == -7).all()


def test_python_joint_runs_the_library_and_survives_a_poisoned_workspace(monkeypatch):
    sc = sc_.slots_scenario(2)
    eng = PyStream(sc)
    out = sc_.run_streams(eng, sc, LogitsEntry(sc.case), bar)
    assert sc_.same_bits(out.results[0], _one())
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", 0xFF)
    ws = eng.jb._ws
    out2 = sc_.run_streams(eng, sc, LogitsEntry(sc.case), bar)  # begin again on the same, now NaN-filled, workspace
    assert eng.jb._ws is ws and sc_.same_bits(out2.results[0], _one())


# ---- end to end ----------------------------------------------------------------------------------------
def _feed_all(dec, x, slot, chunks, other=None):
    dec.start(list(range(dec.S)))
    at = 0
    for i, n in enumerate(chunks):
        mel = torch.zeros(dec.S, 26, x.shape[1], device=DEV)
        fr, fi = [0] * dec.S, [False] * dec.S
        if other is not None:
            for s in range(dec.S):
                mel[s, :4], fr[s] = other[4 * (i % 9): 4 * (i % 9) + 4], 4
        mel[slot, :n] = x[at:at + n]
        fr[slot], fi[slot] = n, i + 1 == len(chunks)
        dec.feed(mel, fr, fi)
        at += n
    return tuple(v[slot].cpu() for v in dec.timed_nbest() + (dec.timed_stable_lengths(), dec.cursors()))


def _decoder(model, slots, beam=3):
    dec = tdt.StreamingTDTBeamDecoder(model, DUR, slots, 26, beam=beam, token_times=True, max_length=40)
    assert dec.es._use_engine and dec.bj.engine and dec.ps._use_engine, "the small model must be one the engine takes"
    return dec


def test_streaming_decoder_chunked_equals_one_shot_and_beam_1_is_greedy():
    model, _ = small_tdt_stream_model(device=DEV, dtype=torch.float32)
    g = torch.Generator().manual_seed(11)
    F = model.encoder.input_norm.num_features
    x, other = torch.randn(26, F, generator=g).to(DEV), torch.randn(40, F, generator=g).to(DEV)
    want = _feed_all(_decoder(model, 1), x, 0, [26])
    assert int(want[1][0]) >= 2
    for chunks in ([2] * 13, [4, 0, 6, 2, 14], [10, 16, 0]):
        got = _feed_all(_decoder(model, 3), x, 2, chunks, other)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes(), (chunks, a, b)
    b1 = _decoder(model, 1, beam=1)
    ids, _, _, fr, _, _, _ = _feed_all(b1, x, 0, [6, 20])
    gr = tdt.StreamingTDTGreedyDecoder(model, DUR, 1, 26, max_symbols_per_frame=1, max_length=64)
    gr.start([0])
    for at, n in ((0, 6), (6, 20)):
        mel = torch.zeros(1, 26, F, device=DEV)
        mel[0, :n] = x[at:at + n]
        gr.feed(mel, [n], [at > 0])
    gi, gf, _ = gr.timed_hypotheses()
    n = int(gr.hypotheses()[1][0])
    assert n >= 2 and int(b1.hypotheses()[1][0]) == n
    assert ids[0, :n].tolist() == gi[0, :n].tolist() and fr[0, :n].tolist() == gf[0, :n].tolist()


def test_transcriber_with_tdt_beam_chunked_audio_equals_one_call():
    model, hp = small_tdt_stream_model(device=DEV, dtype=torch.float32)
    sr = 16000
    audio = fc.signal(1.0, sr, seed=21)
    n = len(audio)

    def run(chunks, slots, slot):
        tr = StreamingTranscriber(model, hp, sr, slots, 3000 if len(chunks) > 1 else n, tdt_durations=DUR, tdt_beam=3, max_length=40,
                                  token_times=True)
        assert isinstance(tr.decoder, tdt.StreamingTDTBeamDecoder) and tr.decoder.bj.engine
        tr.start(list(range(slots)))
        rng, pos = np.random.default_rng(5), 0
        for i, k in enumerate(chunks):
            ks = [int(rng.integers(0, 1501)) for _ in range(slots)]
            ks[slot] = k
            au = torch.tensor(rng.normal(size=(slots, max(ks))).astype(np.float32) * 0.2)
            au[slot, :k] = torch.tensor(audio[pos: pos + k])
            fin = [False] * slots
            fin[slot] = i + 1 == len(chunks)
            tr.feed(au.to(DEV), ks, fin)
            pos += k
        with pytest.raises(RuntimeError, match="log-probabilities"):
            tr.words(slot)
        return tuple(v[slot].cpu() for v in tr.decoder.timed_nbest() + (tr.decoder.timed_stable_lengths(), tr.decoder.cursors()))

    one = run([n], 1, 0)
    assert int(one[1][0]) >= 1
    for a, b in zip(run(fc.ragged_chunks(n, seed=13), 4, 2), one):
        assert a.numpy().tobytes() == b.numpy().tobytes(), (a, b)
    with pytest.raises(ValueError, match="tdt_beam="):
        StreamingTranscriber(model, hp, sr, 1, 3000, beam=4, tdt_durations=DUR)
    with pytest.raises(ValueError, match="tdt_durations"):
        StreamingTranscriber(model, hp, sr, 1, 3000, tdt_beam=4)
