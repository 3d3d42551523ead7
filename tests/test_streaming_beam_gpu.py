"""Streaming beam search on an MI355X, through compute_rnnt_beam_stream_* (decoding.StreamingBeamDecoder and the C ABI): the
offline entry points bit for bit against outputs recorded before the kernels changed, chunking equivalence bitwise in slot k of
16, the offline decoder and the float64 restatement, beam = 1 against streaming greedy, the scripted state machine chunked into
uneven feeds against the offline entry points, the capacity rule with guard regions, stable_lengths, finished and reset slots,
no host read in a feed, and no scratch in the new kernels."""
import math

import numpy as np
import pytest
import torch

from rnnt_speech_recognition_amd import _lib, decoding, joint as jmod
from rnnt_speech_recognition_amd.decoding import StreamingBeamDecoder, StreamingGreedyDecoder
from tests import decode_scripts as ds
from tests import test_greedy_batch_gpu as greedy_gpu
from tests import test_streaming_beam as cpu
from tests.golden import make_beam_offline_goldens as gold
from tests.test_beam_search_gpu import _restate
from tests.test_decode_scripts_gpu import AbiBeam, _dev, _opts
from tests.test_isa_audit import _find, kernels  # noqa: F401  (module-scoped fixture: the built code objects)

DEV = torch.device("cuda:0")


# ---- check 1: the offline entry points, bit for bit ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(gold.CASES)))
def test_offline_entry_points_are_bitwise_what_they_were(case):
    want = np.load(gold.PATH)
    got = gold.run(case)
    for k, v in got.items():
        w = want[f"c{case}_{k}"]
        assert v.shape == w.shape and v.dtype == w.dtype, (case, k)
        assert np.array_equal(gold.bits(v), gold.bits(w)), (case, gold.CASES[case], k)


# One seed per stream (cpu.LENGTHS), chosen on the float64 restatement alone so that every deciding gap of the stream clears twice
# the near-tie bar for K = 1, 4 and 8; check 3 asserts it.  Checks 2 and 3 decode the same streams.
STREAM_SEEDS = {12: [100, 140, 180, 220, 260, 300, 340, 380],
                4096: [106, 152, 180, 220, 286, 313, 343, 407]}


def _gpu_streams(model, vocab, n=len(cpu.LENGTHS)):
    return cpu.seeded_streams(model, cpu.LENGTHS[:n], STREAM_SEEDS[vocab][:n], DEV)


# ---- check 2: chunking equivalence, bitwise -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("vocab", [12, 4096])
@pytest.mark.parametrize("K", [1, 4, 8])
def test_chunked_streams_in_slot_k_of_16_are_bitwise_one_call(vocab, K):
    model = greedy_gpu._decode_model(vocab)
    f = model.encoder.reduce.factor
    X = _gpu_streams(model, vocab)
    N = 24
    assert StreamingBeamDecoder(model, 1, 8, beam=K).bj.engine
    want = [cpu.one_call(model, x, K, N) for x in X]
    assert sum(len(w[0][0]) for w in want) >= 8
    odd = False
    for kind in ["one", "f", "random"]:
        plans, Tc = cpu.plans_for(cpu.LENGTHS, f, kind, 5, cpu.SLOTS)
        odd |= cpu.has_odd_chunk(plans, f)
        got = cpu.run_schedule(model, X, 16, Tc, K, N, plans, seed=len(kind), extra_restart=(2, 11))
        for i in range(len(X)):
            rows, lengths, scores, stable = got[i]
            assert rows == want[i][0] and torch.equal(lengths, want[i][1]) and stable == want[i][3], (kind, i)
            assert torch.equal(scores.view(torch.int32), want[i][2].view(torch.int32)), (kind, i, scores, want[i][2])  # bitwise
    assert odd, "no chunk with an odd number of encoder frames: the schedule does not exercise the buffer-side parity"


# ---- check 3: the offline decoder, the float64 restatement, beam = 1 against greedy --------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("vocab", [12, 4096])
@pytest.mark.parametrize("K", [1, 4, 8])
def test_streams_match_the_offline_decoder_and_a_float64_restatement(vocab, K):
    """The bars of tests/test_beam_search_gpu.py's restatement test: scores within 1e-4 max(1, |s|); a deciding gap is a near-tie
    below 1e-5 (f32-grade joint) / 1e-3 (f16 joint).  Here nothing is skipped: every stream's narrowest gap must clear twice
    that."""
    model = greedy_gpu._decode_model(vocab)
    f = model.encoder.reduce.factor
    lengths = cpu.LENGTHS[:5]
    X = _gpu_streams(model, vocab, 5)
    plans, Tc = cpu.plans_for(lengths, f, "random", 5, cpu.SLOTS)
    got = cpu.run_schedule(model, X, 16, Tc, K, 24, plans, seed=3)
    margin = 1e-5 if vocab <= 32 else 1e-3
    for i, x in enumerate(X):
        with torch.no_grad():
            enc = model.encoder(x[None])
        ids, n, sc = decoding.beam_search_batch(model, enc, torch.tensor([enc.shape[1]], device=DEV), beam=K)
        rows, _, scores, _ = got[i]
        assert rows[0] == ids[0, 0, : int(n[0, 0])].tolist(), i
        want, gap = _restate(model, enc[0], K, vocab > 32)
        print(f"vocab {vocab} K {K} stream {i}: narrowest deciding gap {gap:.3e} (bar {margin:.0e})")
        assert gap > 2 * margin, f"stream {i}: deciding candidates {gap:.3e} apart: pick another seed"
        assert len(rows) == len(want), i
        for k, (y, s) in enumerate(want):
            assert rows[k] == list(y), (i, k)
            assert abs(float(scores[k]) - s) <= 1e-4 * max(1.0, abs(s)), (i, k, float(scores[k]), s)


@pytest.mark.gpu
@pytest.mark.parametrize("vocab", [12, 4096])
def test_beam_one_is_streaming_greedy_with_one_symbol_per_frame(vocab):
    model = greedy_gpu._decode_model(vocab)
    f = model.encoder.reduce.factor
    X = cpu._streams(model, cpu.LENGTHS[:4], 8, DEV)
    plans, Tc = cpu.plans_for(cpu.LENGTHS[:4], f, "random", 2, [2, 0, 3, 1])
    got = cpu.run_schedule(model, X, 4, Tc, 1, 24, plans)
    for i, x in enumerate(X):
        g = StreamingGreedyDecoder(model, 1, x.shape[0], max_length=None, max_symbols_per_frame=1)
        g.start([0])
        g.feed(x[None], [x.shape[0]], [True])
        ids, n, _ = g.hypotheses()
        assert got[i][0][0] == ids[0, : int(n[0])].tolist() and int(got[i][1][0]) == int(n[0]), i


# ---- check 4: the scripted state machine through the stream entry points ------------------------------------------------------
class AbiBeamStream:
    """tests/test_decode_scripts_gpu.py AbiBeam on compute_rnnt_beam_stream_*: the scenario's utterances as streams in B slots,
    their frames delivered in feeds of the uneven lengths `chunks` (cycled); enc = 0 and b1 = 0, so enc_proj = 0 as scripted."""

    H = 8

    def __init__(self, sc, chunks=(3, 1, 4, 2), N=None, poison=False, guard=0):
        self.sc, sj = sc, sc.joint
        self.J, self.V, self.dtype = sj.J, sj.V, sj.dtype
        W2, b2 = sj.weights()
        self.W2, self.b2 = _dev(W2), _dev(b2)
        self.W1, self.b1 = torch.zeros(self.H, self.J, device=DEV), torch.zeros(self.J, device=DEV)
        self.chunks, self.Tc = list(chunks), max(chunks)
        self.N = sc.maxT if N is None else N
        self.left = [min(max(int(v), 0), sc.maxT) for v in sc.frames]
        self.enc = torch.zeros(sc.B, self.Tc, self.H, device=DEV)
        R = sc.B * sc.K
        nbytes = _lib.beam_stream_workspace_bytes(self.Tc, sc.B, sc.K, self.N, self.H, self.J, self.V, self.dtype)
        self.ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=DEV)  # (+ a guard line behind the workspace)
        if poison:
            self.ws.fill_(0xFF)
        self.ws[nbytes:] = 0x5A
        self.nbytes, self.guard = nbytes, guard
        self.parents = torch.full((R,), -7, dtype=torch.int32, device=DEV)
        self.emitted = torch.full((R,), -7, dtype=torch.int32, device=DEV)
        self.rows = torch.empty(R, self.J, device=DEV)
        self.lib = _lib.load()
        self.feeds, self.in_chunk, self.stable = 0, 0, None

    def _o(self):
        return _opts(self.sc.blank, self.Tc)

    def _tail(self):
        sc = self.sc
        return (self.H, self.J, self.V, sc.B, sc.K, self.N, self.dtype, self.ws.data_ptr(), self._o())

    def begin(self):
        _lib.check(self.lib.compute_rnnt_beam_stream_begin(self.W1.data_ptr(), self.b1.data_ptr(), self.W2.data_ptr(),
                                                           self.b2.data_ptr(), *self._tail()), "compute_rnnt_beam_stream_begin")
        self._feed(reset=True)

    def _feed(self, reset=False):
        c = 0 if reset else self.chunks[self.feeds % len(self.chunks)]
        fr = [min(v, c) for v in self.left]
        self.left = [v - u for v, u in zip(self.left, fr)]
        self.in_chunk = c
        self.feeds += 0 if reset else 1
        self._args = (_dev(np.asarray(fr, np.int32)), _dev(np.full(self.sc.B, int(reset), np.int32)),
                      _dev(np.asarray([0 if reset else int(v == 0) for v in self.left], np.int32)))
        cf, rs, fi = self._args
        _lib.check(self.lib.compute_rnnt_beam_stream_feed(self.enc.data_ptr() if c else None, c, cf.data_ptr(), rs.data_ptr(),
                                                          fi.data_ptr(), *self._tail()), "compute_rnnt_beam_stream_feed")

    def step(self, rows):
        if self.in_chunk == 0:
            self._feed()
        self.in_chunk -= 1
        self.rows.copy_(torch.from_numpy(rows))
        _lib.check(self.lib.compute_rnnt_beam_stream_step(self.rows.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(), None,
                                                          None, None, *self._tail()[1:]), "compute_rnnt_beam_stream_step")
        return self.parents.cpu().numpy(), self.emitted.cpu().numpy()

    def results(self):
        sc, g = self.sc, self.guard
        hyps = torch.full((sc.B * sc.K * self.N + 2 * g,), -7, dtype=torch.int32, device=DEV)  # (guard words on both sides)
        lengths = torch.full((sc.B, sc.K), -7, dtype=torch.int32, device=DEV)
        scores = torch.full((sc.B, sc.K), float("nan"), device=DEV)
        stable = torch.full((sc.B,), -7, dtype=torch.int32, device=DEV)
        body = hyps[g: g + sc.B * sc.K * self.N]
        _lib.check(self.lib.compute_rnnt_beam_stream_results(body.data_ptr(), lengths.data_ptr(), scores.data_ptr(), stable.data_ptr(),
                                                             *self._tail()[1:]), "compute_rnnt_beam_stream_results")
        torch.cuda.synchronize()
        assert (hyps[:g] == -7).all() and (hyps[g + body.numel():] == -7).all(), "hyps: written outside [S, K, N]"
        assert (self.ws[self.nbytes:] == 0x5A).all(), "written past the end of the workspace"
        self.stable = stable.cpu().numpy()
        return body.view(sc.B, sc.K, self.N).cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy()


def _script_logits(sc):
    return lambda b, t, y: sc.joint.snap(sc.script(b, t, y))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["merge4", "merge8", "tie5", "tie16", "nothing"])
def test_scripted_scenarios_chunked_equal_the_offline_entry_points(name):
    sc = {"merge4": lambda: ds.merge_scenario(4), "merge8": lambda: ds.merge_scenario(8), "tie5": lambda: ds.tie_scenario(5),
          "tie16": lambda: ds.tie_scenario(16), "nothing": ds.nothing_taken_scenario}[name]()

    class EveryStep:
        """the engine with compute_rnnt_beam[_stream]_results read after begin and after EVERY step (ds.run_beam reads it once,
        at the end): between feeds of uneven length is where the buffer side and the stride-N rows could go wrong"""

        def __init__(self, engine):
            self.engine, self.reads = engine, []

        def begin(self):
            self.engine.begin()
            self.reads.append(self.engine.results())

        def step(self, rows):
            out = self.engine.step(rows)
            self.reads.append(self.engine.results())
            return out

        def results(self):
            return self.engine.results()

    def play(engine):  # no restatement here: engine against engine
        engine = EveryStep(engine)
        trace, ref, _, _ = ds.run_beam(engine, sc.joint, sc.script, sc.B, sc.K, sc.frames, sc.maxT, sc.blank, sc.steps,
                                       _script_logits(sc), sc.ties_allowed, check=False)
        return trace, ref, engine.reads

    offline, ref, off_reads = play(AbiBeam(sc))
    stream, _, str_reads = play(AbiBeamStream(sc, poison=True, guard=64))
    ds.check_expectations(sc, ref.ev)  # (the scenario does what its name says: merges / ties / a carried beam)
    assert len(offline) == sc.steps + 1 and len(off_reads) == len(str_reads) == sc.steps + 1
    for step, (a, b) in enumerate(zip(offline, stream)):  # parents, emitted of every step; then the final ids, lengths, scores
        for p, q in zip(a, b):
            assert p.shape == q.shape and p.dtype == q.dtype and p.tobytes() == q.tobytes(), (name, step)
    assert ds.traces_equal(offline, stream)
    for step, (a, b) in enumerate(zip(off_reads, str_reads)):  # ids, lengths, scores after begin and after every step
        for what, p, q in zip(("ids", "lengths", "scores"), a, b):
            assert p.shape == q.shape and p.dtype == q.dtype and p.tobytes() == q.tobytes(), (name, step, what)
    assert any(r[1].max() > 0 for r in off_reads[1: sc.steps // 2 + 1]), "no tokens in the first half: the reads show nothing"


# ---- check 5: the new rules -----------------------------------------------------------------------------------------------
def _symbol_script(V, blank):
    """every hypothesis prefers the symbol 1 + (t + |y|) % (V - 1) over everything, blank second"""
    def script(b, t, y):
        L = -10.0 - 0.25 * np.arange(V)
        L[blank] = 0.0
        L[1 + (t + len(y) + b) % (V - 1)] = 5.0
        return L
    return script


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,K", [(0, 1), (0, 4), (1, 3)])
def test_capacity_rule_stops_every_hypothesis_at_max_hyp_len(dtype, K):
    V, T, N, blank = 9, 12, 5, 0
    sc = ds.BeamScenario("capacity", dtype, V, 3, K, T, [T, 7, T], blank, _symbol_script(V, blank), T)
    eng = AbiBeamStream(sc, N=N, poison=True, guard=64)
    seqs = [()] * (sc.B * K)
    eng.begin()
    lengths_at = []
    for t in range(T):
        L = np.stack([sc.script(r // K, t, seqs[r]) for r in range(sc.B * K)])
        parents, emitted = eng.step(sc.joint.pred_rows(L))
        for r, (p, e) in enumerate(zip(parents.tolist(), emitted.tolist())):  # a full hypothesis goes on, on blanks alone
            assert e == -1 or len(seqs[p]) < N, (t, r)
        seqs = [seqs[p] + ((e,) if e >= 0 else ()) for p, e in zip(parents.tolist(), emitted.tolist())]
        hyps, lengths, scores = eng.results()  # (guards checked inside, after every frame)
        lengths_at.append(lengths.copy())
        assert lengths.max() <= N
        for b in range(sc.B):
            for k in range(K):
                if math.isfinite(scores[b, k]):
                    assert hyps[b, k, : lengths[b, k]].tolist() == list(seqs[b * K + k]), (t, b, k)
                assert not hyps[b, k, lengths[b, k]:].any()
    final = lengths_at[-1]
    assert (final[0, 0] == N) and (final[2, 0] == N) and final[1, 0] == N  # the best of every slot stopped at N
    assert lengths_at[N - 1][0, 0] == N  # ... after N frames, and stayed there for the other T - N


@pytest.mark.gpu
def test_stable_lengths_on_a_scripted_beam():
    """K = 2: frame 0 splits () into (3) and (); frame 1 merges them into (3) alone; frames 2, 3 diverge behind the shared 3."""
    V, blank = 4, 0

    def script(b, t, y):
        L = np.full(V, -8.0) - 0.1 * np.arange(V)
        if t == 0:
            L[blank], L[3] = 0.0, 6.0
        elif t == 1:
            L[blank if y == (3,) else 3] = 8.0
        elif t == 2:
            L[blank], L[2] = 0.0, 5.0
        else:
            L[blank if len(y) == 2 else 1] = 7.0
        return L

    sc = ds.BeamScenario("stable", 0, V, 2, 2, 4, [4, 2], blank, script, 4)
    eng = AbiBeamStream(sc, chunks=(1, 2, 1), N=6)
    seqs = [()] * 4
    eng.begin()
    eng.results()
    assert eng.stable.tolist() == [0, 0]
    seen = []
    for t in range(4):
        L = np.stack([script(r // 2, t, seqs[r]) for r in range(4)])
        parents, emitted = eng.step(sc.joint.pred_rows(L))
        seqs = [seqs[p] + ((e,) if e >= 0 else ()) for p, e in zip(parents.tolist(), emitted.tolist())]
        hyps, lengths, scores = eng.results()
        rows = [[hyps[b, k, : lengths[b, k]].tolist() for k in range(2) if math.isfinite(scores[b, k])] for b in range(2)]
        assert eng.stable.tolist() == [cpu.common_prefix(r) for r in rows], (t, rows)
        seen.append((eng.stable.tolist(), rows))
    assert [s[0] for s, _ in seen] == [0, 1, 1, 1]  # utterance 0
    assert seen[1][1][0] == [[3]] and sorted(seen[3][1][0]) == [[3, 1], [3, 2]]
    assert [s[1] for s, _ in seen] == [0, 1, 1, 1] and seen[3][1][1] == [[3]]  # utterance 1: frozen after two frames


@pytest.mark.gpu
def test_finished_slots_ignore_feeds_and_resets_leave_neighbours_alone():
    cpu.check_finished_and_reset_slots(greedy_gpu._decode_model(4096), DEV)


@pytest.mark.gpu
def test_poisoned_workspace_decodes_the_same(monkeypatch):
    model = greedy_gpu._decode_model(4096)
    x = cpu._streams(model, [30], 9, DEV)[0]
    fresh = cpu.one_call(model, x, 4, 24)
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", 0xFF)
    poisoned = cpu.one_call(model, x, 4, 24)
    assert fresh[0] == poisoned[0] and torch.equal(fresh[2], poisoned[2]) and fresh[3] == poisoned[3]


@pytest.mark.gpu
def test_a_shape_only_the_stream_refuses_runs_in_torch():
    """2 S K N = 2^31 token words: get_rnnt_beam_stream_workspace_size refuses, and BeamStreamJoint runs its torch mirror."""
    model = greedy_gpu._decode_model(12)
    S, K = 64, 16
    ok, big = jmod.BeamStreamJoint(model.joint, K), jmod.BeamStreamJoint(model.joint, K)
    ok.begin(S, 4, 64)
    big.begin(S, 4, 1 << 20)
    assert ok.engine and not big.engine
    H = model.joint.W1.shape[0]
    big.feed(torch.zeros(S, 2, H, device=DEV), [2] * S, reset=[1] * S, final=None)
    parents, emitted = big.step(pred_proj=torch.zeros(S * K, model.joint.W1.shape[1], device=DEV))
    assert parents.shape == (S * K,) and int((emitted >= 0).sum()) > 0 and big._beams[0]


# ---- check 7: no host read in a feed ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_feed_reads_nothing_from_the_host():
    model = greedy_gpu._decode_model(4096)
    X = cpu._streams(model, [40] * 4, 6, DEV)
    dec = StreamingBeamDecoder(model, 4, 20, beam=4, max_length=32)
    assert dec.es._use_engine and dec.bj.engine and dec.ps._use_engine
    dec.start([0, 1, 2, 3])
    dec.feed(torch.stack([x[:20] for x in X]), [20] * 4, [False] * 4)  # (allocations)
    mel = torch.stack([x[20:] for x in X])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ids, lengths, stable = dec.feed(mel, [20] * 4, [True] * 4)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert decoding.LAST_STEPS == 10
    ref = StreamingBeamDecoder(model, 4, 40, beam=4, max_length=32)
    ref.start([0, 1, 2, 3])
    want = ref.feed(torch.stack(X), [40] * 4, [True] * 4)
    for a, b in zip((ids, lengths, stable), want):
        assert torch.equal(a, b)


# ---- check 8: code objects ------------------------------------------------------------------------------------------------
def test_beam_stream_kernels_use_no_scratch(kernels):
    meta, _ = kernels
    names = (_find(meta, "beam_stream_feed_kernel") + _find(meta, "beam_stream_begin_kernel") + _find(meta, "beam_results_kernel")
             + _find(meta, "beam_select_kernel"))
    assert len(names) == 4
    for k in names + _find(meta, "beam_step_kernel") + _find(meta, "greedy_stream_proj_kernel"):
        assert int(meta[k]["private_segment_fixed_size"]) == 0, k
        assert int(meta[k].get("vgpr_spill_count", "0")) == 0, k
