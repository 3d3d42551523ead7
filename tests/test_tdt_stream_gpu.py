"""Streaming greedy TDT decoding over slots on an MI355X, through the C ABI (compute_rnnt_tdt_greedy_stream_*) and through
tdt.TDTGreedyStreamJoint / tdt.StreamingTDTGreedyDecoder.

Scripted scenarios (tests/tdt_stream_cases.py) run under the comparison rules of tests/tdt_decode_cases.run_tdt: the float64
restatement of each stream's whole utterance is fed with the f32 logits compute_rnnt_joint_logits returns for the hypothesis alone at
alphabet_size = V + D, so ids, frames, lengths, emitted and all_done are compared exactly at every feed and step and nothing is
skipped; scores after n decisions within 2 n 1e-6 max(1, max |lse|) + 2^-23 |s|, hyp_logp within 2e-6 max(1, max |lse|) + 2^-23 |lp|
(profiles/tdt_decode_notes.md).  The equivalence of include/rnnt_tdt_stream.h is checked bit for bit with a real encoder side."""
import types

import numpy as np
import pytest
import torch

from rnnt_speech_recognition_amd import _lib, tdt
from rnnt_speech_recognition_amd.joint import PredictionStep
from tests import tdt_decode_cases as tc
from tests import tdt_stream_cases as cases
from tests.decode_scripts import ScriptedJoint
from tests.test_tdt_greedy_gpu import AbiTdt, LogitsEntry, _dev, _opts, logp_bar, score_bar
from tests.test_tdt_stream import DUR, MEL_CHUNKINGS, chunked, equal_results, small_tdt_stream_model, whole

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C = 16.0
T = 13


class AbiStream:
    """The caller of the C ABI.  times / stats: whether hyp_frames + hyp_logp / logit_stats are given."""

    def __init__(self, S, Tc, V, durations, dtype, blank, cap, W1, b1, W2, b2, poison=False, times=True, stats=True, stream=None):
        self.S, self.Tc, self.V, self.D, self.dtype, self.blank, self.cap = S, Tc, V, len(durations), dtype, blank, cap
        self.H, self.J = W1.shape
        self.times, self.stream = times, stream
        self.W1, self.b1, self.W2, self.b2 = _dev(W1), _dev(b1), _dev(W2), _dev(b2)
        nbytes = _lib.tdt_greedy_stream_workspace_bytes(Tc, S, self.H, self.J, V, self.D, dtype)
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        assert self.ws.data_ptr() % 256 == 0
        if poison:
            self.ws.fill_(0xFF)
        self.lengths = torch.full((S,), -7, dtype=torch.int32, device=DEV)
        self.scores = torch.full((S,), float("nan"), device=DEV)
        self.emitted = torch.full((S,), -7, dtype=torch.int32, device=DEV)
        self.all_done = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        self.stats = torch.full((S, 4), float("nan"), device=DEV) if stats else None
        self.dur = (_lib.ctypes.c_int * self.D)(*durations)
        self.lib = _lib.load_tdtstream()

    def _o(self):
        return _opts(self.blank, self.Tc, self.stream)

    def begin(self, N):
        S = self.S
        self.h = torch.zeros(S, N, dtype=torch.int32, device=DEV)
        self.hf = torch.full((S, N), -1, dtype=torch.int32, device=DEV) if self.times else None
        self.hl = torch.zeros(S, N, device=DEV) if self.times else None
        torch.cuda.synchronize()  # (a side stream: the buffers above were filled on the current one)
        _lib.check(self.lib.compute_rnnt_tdt_greedy_stream_begin(self.W1.data_ptr(), self.b1.data_ptr(), self.W2.data_ptr(),
                                                                 self.b2.data_ptr(), self.H, self.J, self.V, self.dur, self.D, S,
                                                                 self.dtype, self.ws.data_ptr(), self._o()),
                   "compute_rnnt_tdt_greedy_stream_begin")

    def feed(self, enc, frames, reset, final, max_symbols):
        Te = 0 if enc is None else enc.shape[1]
        i32 = lambda x: None if x is None else _dev(np.asarray(x, np.int32))  # noqa: E731
        keep = (None if enc is None else _dev(enc.astype(np.float32)), i32(frames), i32(reset), i32(final), i32(max_symbols))
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        torch.cuda.synchronize()
        _lib.check(self.lib.compute_rnnt_tdt_greedy_stream_feed(ptr(keep[0]), Te, ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(keep[4]),
                                                                self.cap, self.lengths.data_ptr(), self.scores.data_ptr(),
                                                                self.all_done.data_ptr(), self.H, self.J, self.V, self.D, self.S,
                                                                self.dtype, self.ws.data_ptr(), self._o()),
                   "compute_rnnt_tdt_greedy_stream_feed")
        torch.cuda.synchronize()
        return self.lengths.cpu().numpy(), self.scores.cpu().numpy(), int(self.all_done.cpu()[0])

    def step(self, rows):
        rows = _dev(rows.astype(np.float32))
        torch.cuda.synchronize()
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        _lib.check(self.lib.compute_rnnt_tdt_greedy_stream_step(rows.data_ptr(), self.h.data_ptr(), ptr(self.hf), ptr(self.hl),
                                                                self.h.shape[1], self.lengths.data_ptr(), self.scores.data_ptr(),
                                                                self.emitted.data_ptr(), self.all_done.data_ptr(), ptr(self.stats),
                                                                self.J, self.V, self.D, self.S, self.dtype, self.ws.data_ptr(),
                                                                self._o()), "compute_rnnt_tdt_greedy_stream_step")
        torch.cuda.synchronize()
        cpu = lambda x: None if x is None else x.cpu().numpy()  # noqa: E731
        self.last_stats = cpu(self.stats)
        return (cpu(self.emitted), int(self.all_done.cpu()[0]), cpu(self.lengths), cpu(self.scores), cpu(self.h), cpu(self.hf),
                cpu(self.hl))

    def grow(self, N):
        def wider(x, fill):
            y = torch.full((x.shape[0], N), fill, dtype=x.dtype, device=DEV)
            y[:, : x.shape[1]] = x
            return y

        self.h = wider(self.h, 0)
        if self.times:
            self.hf, self.hl = wider(self.hf, -1), wider(self.hl, 0)


class PyStream:
    """The same caller through tdt.TDTGreedyStreamJoint (the engine route)."""

    def __init__(self, S, Tc, durations, dtype, blank, cap, W1, b1, W2, b2):
        joint = types.SimpleNamespace(W1=_dev(W1), b1=_dev(b1), W2=_dev(W2), b2=_dev(b2), blank_label=blank)
        self.S, self.Tc, self.cap = S, Tc, cap
        self.gj = tdt.TDTGreedyStreamJoint(joint, durations, joint_dtype=("f32", "f16")[dtype])
        assert self.gj.engine and self.gj.Jp == W2.shape[0]

    def begin(self, N):
        self.gj.begin(self.S, self.Tc, self.cap, N)

    def feed(self, enc, frames, reset, final, max_symbols):
        self.gj.feed(None if enc is None else _dev(enc.astype(np.float32)), frames, reset, final, max_symbols)
        return self.gj.lengths.cpu().numpy(), self.gj.scores.cpu().numpy(), int(self.gj.all_done.cpu()[0])

    def step(self, rows):
        gj = self.gj
        gj.step(pred_proj=_dev(rows.astype(np.float32)))
        cpu = lambda x: x.cpu().numpy()  # noqa: E731
        return cpu(gj.emitted), int(gj.all_done.cpu()[0]), cpu(gj.lengths), cpu(gj.scores), cpu(gj.hyps), cpu(gj.frames), cpu(gj.logp)

    def grow(self, N):
        while self.gj.hyps.shape[1] < N:
            self.gj.grow_hyps()
        assert self.gj.hyps.shape[1] == N


# ---- scripted scenarios ---------------------------------------------------------------------------
H_SCRIPT = 16


def scripted(sc, dtype):
    """-> (the weights of the scripted joint with W1 = 0 and b1 = 0, the restatement's logits function, pred_row)."""
    sj = ScriptedJoint(64 if dtype == 0 else 128, sc.R, C, dtype)
    W2, b2 = sj.weights()
    keys = max(st.key for st in sc.streams) + 1
    pred_row = lambda key, t, y: sj.pred_rows(sc.script(key, t, y))[0]  # noqa: E731
    case = types.SimpleNamespace(R=sc.R, J=sj.J, dtype=dtype, W2=W2, b2=b2, enc_proj=sj.enc_proj(keys, T), pred_row=pred_row)
    weights = (np.zeros((H_SCRIPT, sj.J), np.float32), np.zeros(sj.J, np.float32), W2, b2)
    return weights, LogitsEntry(case), pred_row


def play(sc, dtype, through="abi", **kw):
    weights, fn, pred_row = scripted(sc, dtype)
    if through == "abi":
        eng = AbiStream(sc.S, sc.Tc, sc.V, sc.durations, dtype, sc.blank, sc.cap, *weights, **kw)
    else:
        eng = PyStream(sc.S, sc.Tc, sc.durations, dtype, sc.blank, sc.cap, *weights)
    garbage = np.random.default_rng(1)  # (W1 = 0: the encoder frames are anything finite)
    out = cases.run_streams(eng, sc, fn, pred_row, lambda key, t0, c: garbage.normal(size=(c, H_SCRIPT)).astype(np.float32), score_bar,
                            logp_bar, min_gap=0.0)
    print(f"dt{dtype} {through}", cases.describe(sc, out))
    return out


SCENARIOS = {"carry": cases.carry_scenario, "cap-at-chunk-end": cases.cap_at_chunk_end_scenario, "budget": cases.budget_scenario,
             "pause": cases.pause_scenario, "phases": cases.phases_scenario, "nan-row": cases.nan_scenario}


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("durations", tc.DURATION_SETS, ids=str)
def test_scripted_chunkings(durations, dtype):
    out = play(cases.chunking_scenario(durations), dtype)
    assert all(r.done[0] for r in out.refs) and sum(len(r.y[0]) for r in out.refs) >= 4
    for res in out.results[1:]:
        assert cases.same_bits(res, out.results[0])


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_scripted_scenarios(name, dtype):
    sc = SCENARIOS[name]()
    out = play(sc, dtype)
    ev = [r.ev for r in out.refs]
    if name == "carry":
        assert out.idle_feeds == [3, 0] and all(4 in e.durations_used and e.jumps_past_end >= 1 for e in ev)
        assert cases.same_bits(out.results[0], out.results[1])
    elif name == "cap-at-chunk-end":
        assert ev[0].capped >= 1 and ev[0].zero_chains >= 2 and ev[0].blank_d0 >= 1 and list(out.refs[0].frames[0]).count(3) == sc.cap
    elif name == "budget":
        assert len(out.refs[0].y[0]) == 3 and out.refs[0].t[0] < 6 and out.refs[1].done[0] and out.refs[1].frames[0][0] == 0
    elif name == "pause":
        assert out.paused_steps >= 2 and all(r.done[0] for r in out.refs)
    elif name == "phases":
        assert not out.refs[1].done[0] and 0 < out.refs[1].t[0] < T and out.refs[3].done[0] and len(out.refs[3].y[0]) > 0
    else:
        assert ev[1].no_finite == 2 and np.isnan(out.results[1][4]) and np.isfinite(out.results[0][4]) and np.isfinite(out.results[2][4])
    # a workspace of 0xFF bytes on entry, and the same decode through the class: bit for bit the same results
    for again in (play(sc, dtype, poison=True), play(sc, dtype, through="class")):
        for a, b in zip(out.results, again.results):
            assert cases.same_bits(a, b)


# ---- the equivalence, bit for bit, with a real encoder side ----------------------------------------
SHAPES = {"dt0-J64": (0, 64, 27), "dt1-J128-two-chunks": (1, 128, 126), "dt1-J128-slice-boundary": (1, 128, 1030), "dt2-J704": (0, 704, 27)}
H_ENC = 16


class RandomSide:
    """Random enc, W1, b1, W2 x 6 and b2 with a blank bias; pred_proj rows by (utterance, tokens so far, last token)."""

    def __init__(self, dtype, J, V, seed, keys=6, blank_bias=1.5):
        rng = np.random.default_rng(seed)
        self.dtype, self.J, self.V, self.seed, self.R = dtype, J, V, seed, V + len(DUR)
        self.W1 = (rng.normal(size=(H_ENC, J)) * 0.5 / np.sqrt(H_ENC)).astype(np.float32)
        self.b1 = (0.1 * rng.normal(size=J)).astype(np.float32)
        self.W2 = ((rng.random((J, self.R)) * 2 - 1) * np.sqrt(6.0 / (J + self.R)) * 6.0).astype(np.float32)
        self.b2 = (0.1 * rng.normal(size=self.R)).astype(np.float32)
        self.b2[0] += blank_bias
        self.enc = rng.normal(size=(keys, 26, H_ENC)).astype(np.float32)

    def weights(self):
        return self.W1, self.b1, self.W2, self.b2

    def pred_row(self, key, y):
        r = np.random.default_rng([self.seed, key, len(y), y[-1] if y else self.R])
        return (0.7 * r.normal(size=self.J)).astype(np.float32)

    def enc_rows(self, key, t0, c):
        return self.enc[key, t0: t0 + c]

    def restatement(self, key, frames=T):
        """The float64 restatement of utterance `key` alone, run to its end -> it (ev.min_gap: the smallest top-two margin), with
        the frames it decided on in .visited."""
        W1, b1, W2, b2 = (x.astype(np.float64) for x in self.weights())
        ep = self.enc[key].astype(np.float64) @ W1 + b1
        fn = lambda b, t, y: np.tanh(ep[t] + self.pred_row(key, y).astype(np.float64)) @ W2 + b2  # noqa: E731
        ref = tc.TDTRestatement(fn, 1, self.V, DUR, [frames], None, 2, frames, 0, min_gap=0.0)
        ref.visited = set()
        while not ref.done[0]:
            ref.visited.add(ref.t[0])
            ref.step(64)
        return ref

    def engine(self, S, Tc=T, **kw):
        return AbiStream(S, Tc, self.V, DUR, self.dtype, 0, 2, *self.weights(), **kw)


def pick_side(dtype, J, V, margin=1e-2):
    """The first seed and blank bias whose utterance 0 shows blanks and tokens with every decision at least `margin` ahead
    (float64).  The wider the vocabulary, the larger the bias at which blanks appear at all."""
    for bias in (1.5, 3.0, 4.5, 6.0):
        for seed in range(40):
            side = RandomSide(dtype, J, V, 1000 * J + V + seed, blank_bias=bias)
            ref = side.restatement(0)
            if ref.ev.min_gap >= margin and ref.ev.blanks >= 2 and len(ref.y[0]) >= 3 and max(ref.ev.durations_used) >= 2:
                return side, ref
    raise AssertionError("no seed with the margin: widen the search, not the margin")


def traffic(key0=1):
    return [cases.Stream(0, key0, 26, [2] * 13), cases.Stream(1, key0 + 1, 26, [3, 1] * 6 + [2], start=1)]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_equivalence_is_bitwise(shape):
    dtype, J, V = SHAPES[shape]
    side, ref = pick_side(dtype, J, V)
    assert ref.ev.blanks >= 2 and len(ref.y[0]) >= 3 and ref.ev.min_gap >= 1e-2  # (conditions on the inputs, asserted: nothing is skipped)
    results = []
    for name, chunks in cases.CHUNKINGS.items():
        alone, _, _ = cases.free_run(side.engine(1), 1, [cases.Stream(0, 0, T, list(chunks))], side.pred_row, side.enc_rows)
        beside, flags, _ = cases.free_run(side.engine(3), 3, traffic() + [cases.Stream(2, 0, T, list(chunks), start=name == "ragged")],
                                          side.pred_row, side.enc_rows)
        results += [alone[0], beside[2]]
        assert len(beside[0][0]) > 0 and len(beside[1][0]) > 0, "the other slots must carry traffic"
    ids, frames, logp, n, score = results[0]
    assert ids.tolist() == list(ref.y[0]) and frames.tolist() == list(ref.frames[0]) and n == len(ref.y[0])
    assert abs(float(score) - ref.score[0]) <= (5e-2 if dtype == 1 else 1e-3) * max(1.0, abs(ref.score[0]))  # (float64 operands: sanity)
    for r in results[1:]:
        assert cases.same_bits(r, results[0]), (shape, r, results[0])
    print(f"[{shape}] tokens={n} blanks={ref.ev.blanks} durations-used={sorted(ref.ev.durations_used)} min-gap={ref.ev.min_gap:.3g} "
          f"jumps-past-end={ref.ev.jumps_past_end}")


def test_a_second_hypothesis_tile_idles_on_a_carry_while_the_first_runs():
    side, ref = pick_side(0, 64, 27)
    skipped = sorted(set(range(max(ref.visited))) - ref.visited)
    assert skipped, "the utterance must jump over a frame: as 1-frame chunks, its slot then idles on the carry"
    alone, _, _ = cases.free_run(side.engine(1), 1, [cases.Stream(0, 0, T, [T])], side.pred_row, side.enc_rows)
    streams = [cases.Stream(s, 1 + s, 26, [2] * 13) for s in range(4)] + [cases.Stream(32, 0, T, [1] * T)]
    got, flags, _ = cases.free_run(side.engine(33, Tc=2), 33, streams, side.pred_row, side.enc_rows)
    assert cases.same_bits(got[4], alone[0])
    assert any(flags[f] == 0 for f in skipped), "tile 0 must run on a feed that finds slot 32 on its carry"


@pytest.mark.parametrize("shape", ["dt0-J64", "dt1-J128-two-chunks"])
def test_one_chunk_equals_the_batched_decoder(shape):
    dtype, J, V = SHAPES[shape]
    side, ref = pick_side(dtype, J, V)
    assert ref.ev.min_gap >= 1e-2  # (the smallest top-two margin of either head, float64: a condition on the inputs)
    got, _, _ = cases.free_run(side.engine(1), 1, [cases.Stream(0, 0, T, [T])], side.pred_row, side.enc_rows)
    ids, frames, logp, n, score = got[0]
    ep = (torch.matmul(_dev(side.enc[:1, :T]), _dev(side.W1)) + _dev(side.b1)).cpu().numpy()
    case = tc.Case("batched", dtype, J, V, DUR, 1, T, [T], None, 2, 0, [64], side.W2, side.b2, ep, None)
    eng = AbiTdt(case)
    eng.begin(64)
    y, flag = (), 0
    while flag == 0:
        out = eng.step(side.pred_row(0, y)[None])
        flag = out[1]
        y = tuple(int(v) for v in out[4][0, : out[2][0]])
    assert flag == 1 and list(y) == ids.tolist() == list(ref.y[0])
    assert out[5][0, :n].tolist() == frames.tolist() == list(ref.frames[0])
    err, bar = abs(float(out[3][0]) - float(score)), score_bar(ref.steps[0], ref.ev.max_lse, float(score))
    print(f"[{shape}] stream score {float(score):.7f} batched {float(out[3][0]):.7f} error {err:.3e} bar {bar:.3e} min-gap {ref.ev.min_gap:.3g}")
    assert err <= bar


# ---- robustness ----------------------------------------------------------------------------------------
def test_optional_outputs_a_side_stream_and_a_poisoned_workspace_change_nothing():
    side, _ = pick_side(1, 128, 126)
    streams = lambda: traffic() + [cases.Stream(2, 0, T, [2, 0, 3, 1, 7])]  # noqa: E731
    base, _, _ = cases.free_run(side.engine(3), 3, streams(), side.pred_row, side.enc_rows)
    variants = {"no-times": dict(times=False), "no-stats": dict(stats=False), "poison": dict(poison=True),
                "side-stream": dict(stream=torch.cuda.Stream())}
    for name, kw in variants.items():
        eng = side.engine(3, **kw)
        got, _, _ = cases.free_run(eng, 3, streams(), side.pred_row, side.enc_rows)
        for i in base:
            a, b = base[i], got[i]
            if name == "no-times":  # hyp_frames = hyp_logp = NULL: the same ids, lengths and scores, bit for bit
                assert b[1] is None and b[2] is None
                a = (a[0], None, None, a[3], a[4])
            assert cases.same_bits(a, b), (name, i)
        if name != "no-stats":
            st = eng.last_stats
            assert st is not None and st.shape == (3, 4)
        else:
            assert eng.last_stats is None


def test_a_nan_encoder_row_costs_its_slot_alone():
    side, _ = pick_side(0, 64, 27)
    streams = lambda: traffic() + [cases.Stream(2, 0, T, [5, 8])]  # noqa: E731
    base, _, _ = cases.free_run(side.engine(3), 3, streams(), side.pred_row, side.enc_rows)
    clean = side.enc.copy()
    at = sorted(side.restatement(2, frames=26).visited)[2]  # (utterance 2 is slot 1's: the third frame it decides on)
    try:
        side.enc[2, at] = np.nan
        got, _, _ = cases.free_run(side.engine(3), 3, streams(), side.pred_row, side.enc_rows)
    finally:
        side.enc[:] = clean
    assert cases.same_bits(got[0], base[0]) and cases.same_bits(got[2], base[2])
    assert np.isnan(got[1][4]) and not np.isnan(base[1][4])


# ---- end to end ----------------------------------------------------------------------------------------
TORCH_ROUTE_BAR = 1e-5  # x max(1, |value|): the bar tests/test_streaming_greedy.py sets for floats that pass through torch's GEMMs


def _decoder(model, slots, route, **kw):
    """A StreamingTDTGreedyDecoder on the engine joint and encoder; route "torch": its prediction network stepped by torch
    (a PredictionStep whose engine is switched off before it begins), "engine": in the library."""
    dec = tdt.StreamingTDTGreedyDecoder(model, DUR, slots, 26, max_symbols_per_frame=2, **kw)
    assert dec.es._use_engine and dec.gj.engine and dec.ps._use_engine, "the small model must be one the engine takes on every route"
    if route == "torch":
        ps = PredictionStep(model.prediction, dec.gj.W1)
        ps.engine = False
        with torch.no_grad():
            dec.ps, dec.pp = ps, ps.begin(slots)
        assert not dec.ps._use_engine
    return dec


@pytest.mark.parametrize("route", ["engine", "torch"])
def test_streaming_decoder_chunked_equals_one_shot(route):
    """Chunked in slot 2 of a 3-slot decoder beside other traffic against one call of a 1-slot decoder.  Prediction network in the
    library: bit for bit.  Prediction network in torch (behind the engine joint): ids, frames and lengths exactly, and the floats
    within 1e-5 max(1, |value|) -- torch's LSTM and its W1 product are rocBLAS GEMMs over all slots' rows, which may round by the
    row count, so pred_proj is not bitwise independent of the number of slots on that route."""
    model, _ = small_tdt_stream_model(device=DEV, dtype=torch.float32)
    g = torch.Generator().manual_seed(11)
    F = model.encoder.input_norm.num_features
    x, other = torch.randn(26, F, generator=g).to(DEV), torch.randn(40, F, generator=g).to(DEV)
    want = whole(_decoder(model, 1, route), x)
    assert want[3] >= 3
    worst = 0.0
    for chunks in MEL_CHUNKINGS:
        xs = x[: sum(chunks)]
        ref = want if sum(chunks) == 26 else whole(_decoder(model, 1, route), xs)
        got = chunked(_decoder(model, 3, route, check_every=3), xs, 2, chunks, other)
        if got[3] == ref[3]:
            worst = max([worst, float((got[4] - ref[4]).abs())] + (got[2] - ref[2]).abs().tolist())
        print(f"[{route}] chunks={chunks} tokens={got[3]} largest float difference so far {worst:.3e}")
        equal_results(got, ref, 0.0 if route == "engine" else TORCH_ROUTE_BAR)
    print(f"[{route}] encoder and joint in the library; tokens={want[3]} frames={want[1].tolist()} largest float difference {worst:.3e}")
