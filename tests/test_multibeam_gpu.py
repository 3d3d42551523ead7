"""The beam search with several symbols per frame on an MI355X, through the C ABI (compute_rnnt_multibeam_*): the scripted scenarios
of tests/multibeam_cases.py, the no-pruning exactness shapes and random joints against the float64 restatement of
include/rnnt_beam_multi.h, fed with the f32 logits compute_rnnt_joint_logits returns for each hypothesis alone.  Ids, lengths,
parents and emitted exactly at every step; scores within decode_scripts.score_bar.  A workspace of 0xFF bytes or of NaNs, a second
run, the batch around an utterance, the prediction route and a HIP-graph replay change nothing.  (Rows are 2 beam per utterance,
an even number: the step kernel's tile edge is crossed at 34 rows, not 33.)"""
import math

import numpy as np
import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib, decoding
from tests import decode_scripts as ds
from tests import multibeam_cases as mc
from tests.test_decode_scripts_gpu import LogitsEntry, _dev, _opts

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SCENARIOS = mc.scenarios()


class AbiMulti:
    """The caller's side of include/rnnt_beam_multi.h.  poison: None, "ff" (a workspace of 0xFF bytes) or "nan" (of f32 NaNs)."""

    def __init__(self, J, V, dtype, W2, b2, enc, frames, B, K, E, N, maxT, blank, poison=None):
        self.J, self.V, self.dtype, self.B, self.K, self.E, self.N, self.maxT, self.blank = J, V, dtype, B, K, E, N, maxT, blank
        self.W2, self.b2, self.enc = _dev(W2), _dev(b2), _dev(enc)
        self.frames = _dev(np.asarray(frames, np.int32))
        R = B * 2 * K
        nbytes = _lib.multibeam_workspace_bytes(maxT, B, K, E, N, J, V, dtype)
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        if poison == "ff":
            self.ws.fill_(0xFF)
        elif poison == "nan":
            self.ws.view(torch.float32).fill_(float("nan"))
        self.parents = torch.full((R,), -7, dtype=torch.int32, device=DEV)
        self.emitted = torch.full((R,), -7, dtype=torch.int32, device=DEV)
        self.rows = torch.empty(R, J, device=DEV)
        self.lib = _lib.load_multibeam()
        self.opts = None

    def _o(self):
        return self.opts if self.opts is not None else _opts(self.blank, self.maxT)

    def begin(self):
        _lib.check(self.lib.compute_rnnt_multibeam_begin(self.enc.data_ptr(), self.frames.data_ptr(), self.W2.data_ptr(),
                                                         self.b2.data_ptr(), self.J, self.V, self.B, self.K, self.E, self.N, self.dtype,
                                                         self.ws.data_ptr(), self._o()), "compute_rnnt_multibeam_begin")

    def enqueue_step(self):
        return self.lib.compute_rnnt_multibeam_step(self.rows.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(), self.J,
                                                    self.V, self.B, self.K, self.E, self.N, self.dtype, self.ws.data_ptr(), self._o())

    def step(self, rows):
        self.rows.copy_(torch.from_numpy(np.ascontiguousarray(rows, np.float32)))
        _lib.check(self.enqueue_step(), "compute_rnnt_multibeam_step")
        return self.parents.cpu().numpy(), self.emitted.cpu().numpy()

    def results(self):
        hyps = torch.full((self.B, self.K, self.N), -7, dtype=torch.int32, device=DEV)
        lengths = torch.full((self.B, self.K), -7, dtype=torch.int32, device=DEV)
        scores = torch.full((self.B, self.K), float("nan"), device=DEV)
        _lib.check(self.lib.compute_rnnt_multibeam_results(hyps.data_ptr(), lengths.data_ptr(), scores.data_ptr(), self.J, self.V, self.B,
                                                           self.K, self.E, self.N, self.dtype, self.ws.data_ptr(), self._o()),
                   "compute_rnnt_multibeam_results")
        return hyps.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy()


def _scripted_engine(sc, poison=None):
    sj = sc.joint
    W2, b2 = sj.weights()
    return AbiMulti(sj.J, sj.V, sj.dtype, W2, b2, sj.enc_proj(sc.B, sc.maxT), sc.frames, sc.B, sc.K, sc.E, sc.max_hyp_len, sc.maxT,
                    sc.blank, poison)


def _run(sc, fn=None, poison=None, check=True):
    fn = fn or LogitsEntry(sc)
    return mc.run_multibeam(_scripted_engine(sc, poison), sc.joint, sc.script, sc.B, sc.K, sc.E, sc.max_hyp_len, sc.frames, sc.maxT,
                            sc.blank, sc.steps, fn, sc.ties_allowed, check=check)


def _both_dtypes():
    cases = []
    for name in mc.NAMES:
        sc = SCENARIOS[name]
        cases.append((name, sc.dtype))
        if sc.dtype == 0:  # (V <= 32 fits the f16 joint too; a scenario written for it may hold more than 32 symbols)
            cases.append((name, 1))
    return cases


@pytest.mark.parametrize("name,dtype", _both_dtypes())
def test_scripted_scenarios(name, dtype):
    import dataclasses

    sc = dataclasses.replace(SCENARIOS[name], dtype=dtype)
    fn = LogitsEntry(sc)
    trace, ref, worst, bar = _run(sc, fn)
    mc.check_expectations(sc, ref)
    print(mc.describe(sc, ref, worst, bar), f"logits-calls={fn.calls}")
    for poison in ("ff", "nan"):
        assert ds.traces_equal(trace, _run(sc, fn, poison, check=False)[0]), f"a workspace of {poison} changed the decode"
    assert ds.traces_equal(trace, _run(sc, fn, check=False)[0]), "two runs differ"


@pytest.mark.parametrize("T,V,E", mc.EXACT_SHAPES)
@pytest.mark.parametrize("dtype", [0, 1])
def test_without_pruning_every_score_is_the_sum_over_alignments(T, V, E, dtype):
    sc = mc.MultiScenario(f"exact-{T}-{V}-{E}", dtype, V, 1, 16, E, T, [T], 0, mc.softmax_script(7 + T, V))
    fn = LogitsEntry(sc)
    trace, ref, worst, bar = _run(sc, fn)
    assert ref.ev.max_candidates <= 16 and ref.ev.max_closed <= 16, "the shape prunes: it cannot show exactness"
    hyps, lengths, scores = trace[-1]
    worst_sum = 0.0
    for k, (y, s) in enumerate(ref.open[0]):
        want = mc.brute_force(fn, 0, T, E, 0, y)
        assert abs(s - want) <= 1e-13 * max(1.0, abs(want))
        err = abs(float(scores[0, k]) - want)
        worst_sum = max(worst_sum, err)
        assert err <= ds.score_bar(sc.steps, ref.ev.max_lse, want), (y, float(scores[0, k]), want)
    print(f"{sc.name} dtype {dtype}: {len(ref.open[0])} hypotheses, worst |score - sum| = {worst_sum:.3e}, "
          f"bar {ds.score_bar(sc.steps, ref.ev.max_lse, 1.0):.3e}")


# ---- random joints -----------------------------------------------------------------------------------
class RandomJoint:
    """A random joint: W2 [J, V], b2, enc_proj [B, T, J]; the pred_proj row of a hypothesis is a random vector by its sequence.
    It stands where run_multibeam wants a ScriptedJoint (V: the row width; pred_rows: the rows as they are)."""

    def __init__(self, seed, J, V, dtype, B, T, scale):
        rng = np.random.default_rng(seed)
        self.J, self.Vout, self.dtype, self.seed = J, V, dtype, seed
        self.W2 = (rng.standard_normal((J, V)) * scale / math.sqrt(J)).astype(np.float32)
        self.b2 = (0.3 * rng.standard_normal(V)).astype(np.float32)
        self.enc = (0.7 * rng.standard_normal((B, T, J))).astype(np.float32)
        self.V, self.c = J, 1.0  # (run_multibeam's junk rows: -0.37 in every unit)

    def pred_rows(self, L):
        return np.ascontiguousarray(L, np.float32)

    def script(self, b, t, y):
        key = [self.seed, len(y), ds.rolling_hash(y, 1000003) % (1 << 31)]
        return (0.7 * np.random.default_rng(key).standard_normal(self.J)).astype(np.float32)


class JointLogits:
    """logits_fn: compute_rnnt_joint_logits for one hypothesis alone (minibatch = maxT = maxU = 1)."""

    def __init__(self, rj):
        self.rj = rj
        self.W2, self.b2 = _dev(rj.W2), _dev(rj.b2)
        self.enc = _dev(rj.enc)
        self.row = torch.empty(rj.J, device=DEV)
        self.out = torch.empty(rj.Vout, device=DEV)
        self.ws = torch.empty(_lib.joint_workspace_bytes(1, 1, 1, rj.J, rj.Vout), dtype=torch.uint8, device=DEV)
        self.cache = {}

    def __call__(self, b, t, y):
        if (b, t, y) not in self.cache:
            rj = self.rj
            self.row.copy_(torch.from_numpy(rj.script(b, t, y)))
            st = _lib.load().compute_rnnt_joint_logits(self.enc[b, t].data_ptr(), self.row.data_ptr(), self.W2.data_ptr(),
                                                       self.b2.data_ptr(), rj.J, rj.Vout, 1, self.out.data_ptr(), rj.dtype,
                                                       self.ws.data_ptr(), _opts(0, 1))
            _lib.check(st, "compute_rnnt_joint_logits")
            self.cache[(b, t, y)] = self.out.cpu().numpy().copy()
        return self.cache[(b, t, y)]


# (J, V, dtype, B, K, E, T, frames, blank): V = 12 and V = 4096 / J = 640; beam 1, 4, 16; 32, 34 and 288 rows; T = 1 and ragged; E = 1, 3
RANDOM_CASES = [
    (64, 12, 0, 4, 4, 3, 3, [3, 1, 0, 2], 0),        # 32 rows: one full tile
    (64, 12, 0, 17, 1, 3, 2, [2] * 16 + [1], 11),    # 34 rows: a second tile of two rows; beam 1
    (64, 12, 0, 9, 16, 1, 2, [2, 1, 2, 0, 2, 2, 1, 2, 2], 0),   # 288 rows; beam 16
    (64, 12, 0, 2, 4, 1, 1, [1, 1], 5),              # T = 1
    (640, 4096, 1, 2, 4, 3, 2, [2, 1], 0),           # the f16 joint at the flagship width
    (640, 4096, 1, 1, 16, 1, 2, [2], 4095),
]


@pytest.mark.parametrize("case", RANDOM_CASES, ids=lambda c: f"J{c[0]}-V{c[1]}-B{c[3]}-K{c[4]}-E{c[5]}-T{c[6]}")
def test_random_joint_against_the_restatement(case):
    J, V, dtype, B, K, E, T, frames, blank = case
    rj = RandomJoint(1000 + V + B + K, J, V, dtype, B, T, 6.0 if V > 100 else 3.0)
    fn = JointLogits(rj)
    N = T * E

    def engine(poison=None):
        return AbiMulti(J, V, dtype, rj.W2, rj.b2, rj.enc, frames, B, K, E, N, T, blank, poison)

    trace, ref, worst, bar = mc.run_multibeam(engine(), rj, rj.script, B, K, E, N, frames, T, blank, T * (E + 1), fn)
    print(f"random joint {case[:7]}: lists <= {ref.ev.max_candidates}/{ref.ev.max_closed}, merges {ref.ev.closed_merges}, "
          f"min gap {ref.ev.min_gap:.3e}, worst score error {worst:.3e} (bar {bar:.3e})")
    again = mc.run_multibeam(engine("ff"), rj, rj.script, B, K, E, N, frames, T, blank, T * (E + 1), fn, check=False)[0]
    assert ds.traces_equal(trace, again), "a workspace of 0xFF bytes changed the decode"
    # utterance 0 alone: the same bits as inside the batch
    solo = mc.run_multibeam(AbiMulti(J, V, dtype, rj.W2, rj.b2, rj.enc[:1], frames[:1], 1, K, E, N, T, blank), rj, rj.script, 1, K, E,
                            N, frames[:1], T, blank, T * (E + 1), fn, check=False)[0]
    for (p1, e1), (pB, eB) in zip(solo[:-1], trace[:-1]):
        assert np.array_equal(p1, pB[: 2 * K]) and np.array_equal(e1, eB[: 2 * K])
    for x1, xB in zip(solo[-1], trace[-1]):
        assert np.array_equal(x1[0], xB[0])


def test_a_graph_replay_of_a_step_equals_the_direct_call():
    sc = SCENARIOS["merges"]
    sj = sc.joint
    s = 4  # the captured step: round 1 of frame 1

    def rows_for(eng, upto):
        """Drive `eng` through steps [0, upto) directly -> the rows of step `upto`."""
        KR = 2 * sc.K
        seqs = [()] * (sc.B * KR)
        eng.begin()
        for step in range(upto + 1):
            L = np.stack([sc.script(r // KR, step // (sc.E + 1), seqs[r]) for r in range(sc.B * KR)])
            rows = sj.pred_rows(L)
            if step == upto:
                return rows
            p, e = eng.step(rows)
            seqs = [seqs[q] + ((v,) if v >= 0 else ()) for q, v in zip(p.tolist(), e.tolist())]

    direct = _scripted_engine(sc)
    rows = rows_for(direct, s)
    want = direct.step(rows) + direct.results()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):  # first use outside the capture, on the stream's own options
        eng = _scripted_engine(sc)
        rows2 = rows_for(eng, s)
        assert np.array_equal(rows, rows2)
        eng.rows.copy_(torch.from_numpy(rows2))
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, sc.blank, sc.maxT, 1)
        assert eng.enqueue_step() == 0
    eng.opts = None
    eng.parents.fill_(-7)
    eng.emitted.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    got = (eng.parents.cpu().numpy(), eng.emitted.cpu().numpy()) + eng.results()
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("vocab,E", [(12, 1), (12, 3), (4096, 2)])
def test_both_prediction_routes_give_the_same_ids(vocab, E):
    """decoding.beam_search_batch(symbols_per_frame=E) on the engine, with the prediction network stepped by torch and by the
    library (as tests/test_prednet_step_gpu.py compares the modified search's routes)."""
    from rnnt_speech_recognition_amd import joint as jmod
    from tests.test_greedy_batch_gpu import _decode_model

    model = _decode_model(vocab)
    assert jmod.MultiBeamJoint(model.joint, 4, E).engine
    torch.manual_seed(18)
    B = 6
    mel = torch.randn(B, 24, 8).to(DEV)
    sl = torch.tensor([24, 19, 24, 4, 0, 13], device=DEV)
    with torch.no_grad():
        enc = model.encoder(mel)
    frames = pkg.reduced_lengths(sl, model.hp.time_reduction_factor)
    a = decoding.beam_search_batch(model, enc, frames, beam=4, symbols_per_frame=E)
    ids, lengths, scores = decoding.beam_search_batch(model, enc, frames, beam=4, prediction="engine", symbols_per_frame=E)
    T = enc.shape[1]
    assert ids.shape == (B, 4, T * E) and ids.is_cuda and ids.dtype == torch.int32 and scores.dtype == torch.float32
    assert torch.equal(a[0], ids) and torch.equal(a[1], lengths)
    fin = torch.isfinite(a[2])
    assert torch.equal(fin, torch.isfinite(scores))
    assert ((a[2][fin] - scores[fin]).abs() <= 1e-4 * a[2][fin].abs().clamp(min=1)).all()
    best = decoding.beam_decode_batch(model, mel, sl, beam=4, symbols_per_frame=E)
    assert torch.equal(best[0], ids[:, 0]) and torch.equal(best[1], lengths[:, 0])
    assert int(lengths[4, 0]) == 0 and float(scores[4, 0]) == 0.0  # no frames: [((), 0)]
