"""Streaming beam search with several symbols per frame on an MI355X, through the C ABI (compute_rnnt_multibeam_stream_*): the
scenarios of tests/multibeam_stream_cases.py against the float64 restatement of include/rnnt_beam_multi.h run over each stream's
whole utterance, fed with the f32 logits compute_rnnt_joint_logits returns for each hypothesis alone.  parents and emitted exactly at
every step; ids, lengths, frames and both stable lengths exactly; scores within decode_scripts.score_bar(rounds taken, max |lse|,
s).  Bitwise: every chunking against the one-chunk 1-slot run, each slot position against slot 0, timed against untimed, the stream
against compute_rnnt_multibeam_* offline on enc_proj = b1, a workspace of 0xFF bytes or of NaNs, a second run, a HIP-graph replay.
The shapes are the smallest at which the kernels can go wrong: 2, 32, 34 and 288 rows; one and two vocabulary slices; E = 1, 2, 3, 8;
max_chunk_frames = 1."""
import numpy as np
import pytest
import torch

from rnnt_speech_recognition_amd import _lib, decoding
from rnnt_speech_recognition_amd import joint as jmod
from tests import decode_scripts as ds
from tests import multibeam_stream_cases as sc_
from tests.test_decode_scripts_gpu import LogitsEntry, _dev, _opts
from tests.test_multibeam_gpu import AbiMulti

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
JOINTS = {"f32-V12": dict(dtype=0, V=12), "f16-V12": dict(dtype=1, V=12), "f16-V130": dict(dtype=1, V=130, J=256)}
_LOGITS = {}  # (J, V, dtype) -> the logits cache (rows are bitwise reproducible)


def logits_fn(sc):
    fn = LogitsEntry(sc)
    fn.cache = _LOGITS.setdefault((sc.joint.J, sc.V, sc.dtype), {})
    return fn


class AbiStream:
    """The caller's side of include/rnnt_beam_multi_stream.h.  poison: None, "ff" (a workspace of 0xFF bytes) or "nan" (of f32 NaNs)."""

    def __init__(self, sc, timed=True, poison=None):
        sj = sc.joint
        self.sc, self.J, self.V, self.dtype, self.timed = sc, sj.J, sj.V, sj.dtype, int(timed)
        W2, b2 = sj.weights()
        self.W2, self.b2 = _dev(W2), _dev(b2)
        self.W1, self.b1 = torch.zeros(sc_.H, sj.J, device=DEV), torch.zeros(sj.J, device=DEV)
        R = sc.S * 2 * sc.K
        nbytes = _lib.multibeam_stream_workspace_bytes(sc.Tc, sc.S, sc.K, sc.E, sc.N, sc_.H, self.J, self.V, self.dtype, timed)
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        if poison == "ff":
            self.ws.fill_(0xFF)
        elif poison == "nan":
            self.ws.view(torch.float32).fill_(float("nan"))
        self.parents = torch.full((R,), -7, dtype=torch.int32, device=DEV)
        self.emitted = torch.full((R,), -7, dtype=torch.int32, device=DEV)
        self.rows = torch.empty(R, self.J, device=DEV)
        self.lib = _lib.load_multibeam_stream()
        self.opts = None
        self.sizes = (sc.S, sc.K, sc.E, sc.N, self.dtype, self.timed)

    def _o(self):
        return self.opts if self.opts is not None else _opts(self.sc.blank, self.sc.Tc)

    def begin(self):
        _lib.check(self.lib.compute_rnnt_multibeam_stream_begin(self.W1.data_ptr(), self.b1.data_ptr(), self.W2.data_ptr(),
                                                                self.b2.data_ptr(), sc_.H, self.J, self.V, *self.sizes,
                                                                self.ws.data_ptr(), self._o()), "compute_rnnt_multibeam_stream_begin")

    def feed(self, enc, fr, rs, fi):
        Te = 0 if enc is None else enc.shape[1]
        self._keep = (None if enc is None else _dev(enc), _dev(np.asarray(fr, np.int32)), _dev(np.asarray(rs, np.int32)),
                      _dev(np.asarray(fi, np.int32)))
        e, f, r, l = self._keep
        _lib.check(self.lib.compute_rnnt_multibeam_stream_feed(None if e is None else e.data_ptr(), Te, f.data_ptr(), r.data_ptr(),
                                                               l.data_ptr(), sc_.H, self.J, self.V, *self.sizes, self.ws.data_ptr(),
                                                               self._o()), "compute_rnnt_multibeam_stream_feed")

    def enqueue_step(self):
        return self.lib.compute_rnnt_multibeam_stream_step(self.rows.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(),
                                                           self.J, self.V, *self.sizes, self.ws.data_ptr(), self._o())

    def step(self, rows):
        self.rows.copy_(torch.from_numpy(np.ascontiguousarray(rows, np.float32)))
        _lib.check(self.enqueue_step(), "compute_rnnt_multibeam_stream_step")
        return self.parents.cpu().numpy(), self.emitted.cpu().numpy()

    def results(self):
        S, K, N = self.sc.S, self.sc.K, self.sc.N
        hyps = torch.full((S, K, N), -7, dtype=torch.int32, device=DEV)
        lengths = torch.full((S, K), -7, dtype=torch.int32, device=DEV)
        scores = torch.full((S, K), float("nan"), device=DEV)
        stable = torch.full((S,), -7, dtype=torch.int32, device=DEV)
        frames = torch.full((S, K, N), -7, dtype=torch.int32, device=DEV) if self.timed else None
        tstable = torch.full((S,), -7, dtype=torch.int32, device=DEV) if self.timed else None
        _lib.check(self.lib.compute_rnnt_multibeam_stream_results(
            hyps.data_ptr(), lengths.data_ptr(), scores.data_ptr(), stable.data_ptr(), _lib.ptr(frames), _lib.ptr(tstable), self.J,
            self.V, *self.sizes, self.ws.data_ptr(), self._o()), "compute_rnnt_multibeam_stream_results")
        return tuple(None if x is None else x.cpu().numpy() for x in (hyps, lengths, scores, stable, frames, tstable))


def _score_ok(got, want, rounds, ref):
    return abs(got - want) <= ds.score_bar(rounds, ref.ev.max_lse, want)


def _run(sc, timed=True, poison=None):
    out = sc_.run_streams(AbiStream(sc, timed, poison), sc, logits_fn(sc), _score_ok)
    sc_.check_expectations(sc, out)
    return out


def _scenario(kind, joint):
    j = JOINTS[joint]
    kw = dict(dtype=j["dtype"], V=j["V"], J=j.get("J", 0))
    if kind == "cuts":
        return sc_.chunking_scenario("cuts", **kw)
    if kind == "frame-merge":
        return sc_.frame_merge_scenario(**kw)
    if kind == "overflow-boundary":
        return sc_.overflow_boundary_scenario(lambda sc: (lambda key, t, y: sc.joint.snap(sc.script(key, t, y))), **kw)
    if kind == "slots":
        return sc_.slots_scenario(2, **kw)
    if kind == "final":
        return sc_.final_scenario(**kw)
    raise KeyError(kind)


@pytest.mark.parametrize("joint", list(JOINTS))
@pytest.mark.parametrize("kind", ["cuts", "frame-merge", "overflow-boundary", "slots", "final"])
def test_scenarios_on_each_joint(kind, joint):
    sc = _scenario(kind, joint)
    out = _run(sc)
    print(sc_.describe(sc, out))


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("make", [lambda d: sc_.capacity_scenario(3, dtype=d), lambda d: sc_.capacity_scenario(1, dtype=d),
                                  lambda d: sc_.empty_turn_scenario(dtype=d), lambda d: sc_.nan_rows_scenario(dtype=d),
                                  lambda d: sc_.ties_scenario(dtype=d)], ids=["capacity-3", "capacity-1", "empty-turn", "nan-rows", "ties"])
def test_rule_scenarios(make, dtype):
    sc = make(dtype)
    out = _run(sc)
    print(sc_.describe(sc, out))


# (S, K, slot, E, joint, Tc): 2, 32, 34 and 288 rows; E = 8, 2, 3, 1; max_chunk_frames = 1; two vocabulary slices
GEOMETRY = [(1, 1, 0, 8, "f32-V12", 1), (4, 4, 1, 2, "f32-V12", 4), (17, 1, 16, 3, "f32-V12", 4), (9, 16, 4, 1, "f32-V12", 4),
            (4, 4, 3, 2, "f16-V12", 4), (4, 4, 0, 3, "f16-V130", 4)]


@pytest.mark.parametrize("case", GEOMETRY, ids=lambda c: f"S{c[0]}-K{c[1]}-E{c[3]}-{c[4]}-Tc{c[5]}")
def test_row_geometry(case):
    S, K, slot, E, joint, Tc = case
    j = JOINTS[joint]
    sc = sc_.geometry_scenario(S, K, slot, E=E, dtype=j["dtype"], V=j["V"], J=j.get("J", 0), Tc=Tc, chunks=[1] * 4 if Tc == 1 else (1, 2, 1),
                               blank=j["V"] - 1 if j["V"] > 128 else 0)
    out = _run(sc)
    print(sc_.describe(sc, out))
    solo = _run(sc_.geometry_scenario(1, K, 0, E=E, dtype=j["dtype"], V=j["V"], J=j.get("J", 0), Tc=4, chunks=[4],
                                      blank=j["V"] - 1 if j["V"] > 128 else 0))
    assert sc_.same_bits(solo.results[0], out.results[0]), "the stream depends on its slot, its chunking or the streams around it"


@pytest.mark.parametrize("dtype", [0, 1])
def test_chunkings_slots_timed_and_offline_agree_bitwise(dtype):
    V = 12
    one = _run(sc_.chunking_scenario("one", dtype=dtype, V=V)).results[0]
    for name in sc_.CHUNKINGS:
        if name != "one":
            assert sc_.same_bits(one, _run(sc_.chunking_scenario(name, dtype=dtype, V=V)).results[0]), name
    untimed = _run(sc_.chunking_scenario("cuts", dtype=dtype, V=V), timed=False).results[0]
    assert sc_.same_bits(one[:4], untimed[:4]) and untimed[4] is None and untimed[5] is None
    for slot in range(4 if dtype == 0 else 1):
        assert sc_.same_bits(one, _run(sc_.slots_scenario(slot, dtype=dtype, V=V)).results[0]), ("slot", slot)
    # the offline search on enc_proj = b1 = 0, driven by the same caller's rules
    sc = sc_.chunking_scenario("one", dtype=dtype, V=V)
    sj, T, K, E = sc.joint, sc_.T13, sc.K, sc.E
    W2, b2 = sj.weights()
    eng = AbiMulti(sj.J, sj.V, sj.dtype, W2, b2, sj.enc_proj(1, T), [T], 1, K, E, sc.N, T, sc.blank)
    eng.begin()
    seqs = [()] * (2 * K)
    for step in range(T * (E + 1)):
        rows = np.stack([sj.pred_rows(sc.script(0, step // (E + 1), y))[0] for y in seqs])
        p, e = eng.step(rows)
        seqs = [seqs[q] + ((v,) if v >= 0 else ()) for q, v in zip(p.tolist(), e.tolist())]
    hyps, lengths, scores = eng.results()
    assert sc_.same_bits((hyps[0], lengths[0], scores[0]), one[:3]), "the stream is not the offline search"


@pytest.mark.parametrize("joint", ["f32-V12", "f16-V130"])
def test_a_poisoned_workspace_and_a_second_run_change_nothing(joint):
    sc = _scenario("slots", joint)
    first = _run(sc)
    for poison in ("ff", "nan", None):
        again = _run(sc, poison=poison)
        assert ds.traces_equal(first.trace, again.trace), poison
        for a, b in zip(first.results, again.results):
            assert sc_.same_bits(a, b), poison


def test_a_graph_replay_of_a_step_equals_the_direct_call():
    sc = sc_.chunking_scenario("one", V=12)
    sj, KR, s = sc.joint, 2 * sc.K, 4  # the captured step: round 1 of frame 1

    def rows_for(eng, upto):
        """Drive `eng` through steps [0, upto) directly -> the rows of step `upto`."""
        seqs = [()] * KR
        eng.begin()
        eng.feed(np.zeros((1, sc_.T13, sc_.H), np.float32), [sc_.T13], [1], [1])
        for step in range(upto + 1):
            rows = sj.pred_rows(np.stack([sc.script(0, step // (sc.E + 1), y) for y in seqs]))
            if step == upto:
                return rows
            p, e = eng.step(rows)
            seqs = [seqs[q] + ((v,) if v >= 0 else ()) for q, v in zip(p.tolist(), e.tolist())]

    direct = AbiStream(sc)
    rows = rows_for(direct, s)
    want = direct.step(rows) + direct.results()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):  # first use outside the capture, on the stream's own options
        eng = AbiStream(sc)
        rows2 = rows_for(eng, s)
        assert np.array_equal(rows, rows2)
        eng.rows.copy_(torch.from_numpy(rows2))
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, sc.blank, sc.Tc, 1)
        assert eng.enqueue_step() == 0
    eng.opts = None
    eng.parents.fill_(-7)
    eng.emitted.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    got = (eng.parents.cpu().numpy(), eng.emitted.cpu().numpy()) + eng.results()
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("E", [1, 3])
def test_the_streaming_decoder_on_the_engine_follows_the_cpu_mirror(E):
    """decoding.StreamingMultiBeamDecoder on the engine (joint, prediction network and encoder in the library) against the same
    decoder on CPU tensors at V = 12: same ids and lengths, scores within 1e-4 max(1, |s|), the bar of the offline test."""
    from tests.test_greedy_batch_gpu import _decode_model

    model = _decode_model(12)
    f = int(model.encoder.reduce.factor)
    torch.manual_seed(18)
    S, T = 3, 12 * f
    mel = torch.randn(S, T, 8)
    cpu = _decode_model(12).cpu()
    cpu.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    outs = []
    for m, dev in ((model, DEV), (cpu, torch.device("cpu"))):
        dec = decoding.StreamingMultiBeamDecoder(m, S, 6 * f, beam=4, symbols_per_frame=E, max_length=12 * E, token_times=True)
        assert dec.bj.engine == (dev.type == "cuda") and isinstance(dec.bj, jmod.MultiBeamStreamJoint)
        dec.start([0, 2])
        for lo, fin in ((0, False), (6 * f, True)):
            chunk = mel[:, lo: lo + 6 * f].to(dev)
            dec.feed(chunk, [6 * f, 0, 4 * f], [fin, False, fin])
        outs.append(tuple(x.cpu() for x in dec.timed_nbest()) + (dec.timed_stable_lengths().cpu(),))
    (ids, lengths, scores, frames, ts), (ids2, lengths2, scores2, frames2, ts2) = outs
    assert torch.equal(ids, ids2) and torch.equal(lengths, lengths2) and torch.equal(frames, frames2) and torch.equal(ts, ts2)
    fin = torch.isfinite(scores2)
    assert torch.equal(fin, torch.isfinite(scores)) and not fin[1].any()  # (slot 1 was never started)
    assert ((scores[fin].double() - scores2[fin].double()).abs() <= 1e-4 * scores2[fin].double().abs().clamp(min=1)).all()
