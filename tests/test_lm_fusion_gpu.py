"""N-gram LM shallow fusion on an MI355X, through the C ABI: the four compute_rnnt_beam_*_step_lm entry points of include/rnnt_lm.h
(libwarprnnt_lm.so, on workspaces that libwarprnnt.so begins, feeds and reads) against the float64 restatement of rules 2' and 3'
(tests/lm_cases.py), fed with the f32 logits compute_rnnt_joint_logits returns for each hypothesis alone.  Ids, lengths, parents,
emitted and lm_states exactly at every step; scores within n 1e-6 max(1, max |lse|) + 2^-23 |s|, |s| including the LM."""
import ctypes
import math

import numpy as np
import pytest
import torch

from rnnt_speech_recognition_amd import _lib
from rnnt_speech_recognition_amd.lm import NgramLM
from tests import bias_cases as bc
from tests import decode_scripts as ds
from tests import lm_cases as lc
from tests.lm_cases import BOS
from tests.test_context_bias_gpu import Twin
from tests.test_decode_scripts_gpu import LogitsEntry, _dev, _opts

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = ("beam", "timed", "stream", "stream_timed")


class LmTwin(Twin):
    """test_context_bias_gpu.Twin with the step of libwarprnnt_lm.so: graph an NgramLM, "null" (graph == NULL) or None (the
    unfused entry of libwarprnnt.so)."""

    def _call(self, what, *args):
        if what == "step_biased":
            what, lib = "step_lm", _lib.load_lm()
        else:
            lib = self.lib
        _lib.check(getattr(lib, self._name(what))(*args), self._name(what))


def _play(name_or_sc, kind="beam", chunk=None):
    sc = lc.SCENARIOS[name_or_sc]() if isinstance(name_or_sc, str) else name_or_sc
    g = lc.build_lm(sc)
    engine = LmTwin(sc, kind, g, chunk)
    trace, ref, worst, bar = lc.run_lm(engine, sc.joint, sc.script, g, sc.B, sc.K, sc.frames, sc.maxT, sc.blank, sc.steps,
                                       LogitsEntry(sc), sc.ties_allowed)
    ds.check_expectations(sc, ref.ev)
    print(f"[{sc.name} {kind} J={sc.joint.J} dtype={sc.dtype}] states={g.num_states} arcs={g.num_arcs} merges={ref.ev.merges} "
          f"ties={ref.ev.ties} carried={ref.ev.carried} min-gap={ref.ev.min_gap:.3g} score-error={worst:.3e} bar={bar:.3e}")
    return sc, trace, ref, g, engine


@pytest.mark.parametrize("name", sorted(lc.SCENARIOS))
def test_scripted_scenarios_against_the_restatement(name):
    """flip0 / depth / K1 ...: beam_step_lm_kernel<0>; flip1 / ties2 / merges3 / K4 ...: <1> (binary16 operands); flip2: <2> (J = 704)."""
    sc, _, ref, g, _ = _play(name)
    lc.check_scenario(name, sc, ref, g)


def test_several_vocabulary_slices_and_a_large_lm():
    """V = 384 (three slices of 128 symbols), J = 128, random weights; a trigram LM estimated from random sequences over 56 of the
    symbols: an arc on every non-blank symbol at E, more than 2,000 states, scores that are no dyadic numbers.  The restatement
    reads compute_rnnt_joint_logits per (utterance, frame, last token)."""
    J, V, B, K, T, blank = 128, 384, 2, 4, 6, 0
    rng = np.random.default_rng(5)
    sub = rng.permutation(np.arange(1, V))[:56]
    seqs = [[int(x) for x in rng.choice(sub, size=int(rng.integers(4, 12)))] for _ in range(1400)]
    g = NgramLM.estimate(seqs, 3, blank, V, discount=0.7)
    assert g.num_states >= 2000 and g.arc_offsets[2] - g.arc_offsets[1] == V - 1 and g.empty_state == 1
    W2 = (rng.standard_normal((J, V)) * 0.4).astype(np.float32)
    b2 = (rng.standard_normal(V) * 0.2).astype(np.float32)
    enc = (rng.standard_normal((B, T, J)) * 0.7).astype(np.float32)
    emb = (rng.standard_normal((V + 1, J)) * 0.7).astype(np.float32)  # pred_proj by the last token (V: none yet)
    dW2, db2, denc = _dev(W2), _dev(b2), _dev(enc)
    lib, llib = _lib.load(), _lib.load_lm()
    out, row, frame = torch.empty(V, device=DEV), torch.empty(J, device=DEV), torch.empty(J, device=DEV)
    ws1 = torch.empty(_lib.joint_workspace_bytes(1, 1, 1, J, V), dtype=torch.uint8, device=DEV)
    cache = {}

    def logits_fn(b, t, y):
        key = (b, t, y[-1] if y else V)
        if key not in cache:
            row.copy_(torch.from_numpy(emb[key[2]]))
            frame.copy_(denc[b, t])
            _lib.check(lib.compute_rnnt_joint_logits(frame.data_ptr(), row.data_ptr(), dW2.data_ptr(), db2.data_ptr(),
                                                     J, V, 1, out.data_ptr(), 1, ws1.data_ptr(), _opts(0, 1)), "compute_rnnt_joint_logits")
            cache[key] = out.cpu().numpy().copy()
        return cache[key]

    frames = [T, T - 2]
    ref = lc.LmBeamRestatement(logits_fn, g, B, K, frames, T, blank)
    ws = torch.full((_lib.beam_workspace_bytes(T, B, K, J, V, 1),), 0xFF, dtype=torch.uint8, device=DEV)
    o = _opts(blank, T)
    dfr = _dev(np.asarray(frames, np.int32))
    _lib.check(lib.compute_rnnt_beam_begin(denc.data_ptr(), dfr.data_ptr(), dW2.data_ptr(), db2.data_ptr(), J, V, B, K, 1, ws.data_ptr(), o),
               "compute_rnnt_beam_begin")
    R = B * K
    parents, emitted, states = (torch.full((R,), -7, dtype=torch.int32, device=DEV) for _ in range(3))
    last = [V] * R
    rows = torch.empty(R, J, device=DEV)
    deep = 0
    for t in range(T):
        rows.copy_(torch.from_numpy(emb[last]))
        _lib.check(llib.compute_rnnt_beam_step_lm(rows.data_ptr(), parents.data_ptr(), emitted.data_ptr(), None, None, None, J, V, B, K,
                                                  1, ws.data_ptr(), o, g.byref(DEV), states.data_ptr()), "compute_rnnt_beam_step_lm")
        want_p, want_e, want_q = ref.step()
        p, e = parents.cpu().tolist(), emitted.cpu().tolist()
        assert (p, e, states.cpu().tolist()) == (want_p, want_e, want_q), t
        last = [x if x >= 0 else last[src] for src, x in zip(p, e)]
        deep += sum(int(g.depth[q]) == 2 for q in want_q)
    assert deep > 0, "no slot at a state of two tokens: the case shows nothing of the chain"
    hyps, lengths, scores = torch.empty(B, K, T, dtype=torch.int32, device=DEV), torch.empty(B, K, dtype=torch.int32, device=DEV), \
        torch.empty(B, K, device=DEV)
    _lib.check(lib.compute_rnnt_beam_results(hyps.data_ptr(), lengths.data_ptr(), scores.data_ptr(), J, V, B, K, 1, ws.data_ptr(), o),
               "compute_rnnt_beam_results")
    for b in range(B):
        for k, (y, s, _) in enumerate(ref.beams[b]):
            assert hyps[b, k, : len(y)].tolist() == list(y) and int(lengths[b, k]) == len(y)
            err, bar = abs(float(scores[b, k]) - s), ds.score_bar(frames[b], ref.ev.max_lse, s)
            print(f"  score b={b} k={k}: error {err:.3e} bar {bar:.3e}")
            assert err <= bar, (b, k)
    print(f"[V384] states={g.num_states} arcs={g.num_arcs} min-gap={ref.ev.min_gap:.3g} slots-at-depth-2={deep}")


def _trace(sc, kind, graph, chunk=None):
    """Engine alone (no restatement): everything every step and the results return."""
    engine = LmTwin(sc, kind, graph, chunk)
    engine.begin()
    seqs, out = [()] * (sc.B * sc.K), []
    for step in range(sc.steps):
        L = np.stack([sc.script(r // sc.K, step, seqs[r]) for r in range(sc.B * sc.K)])
        p, e, q = engine.step(sc.joint.pred_rows(L))
        seqs = [seqs[a] + ((b,) if b >= 0 else ()) for a, b in zip(p.tolist(), e.tolist())]
        out.append((p.copy(), e.copy()) + ((q.copy(),) if graph is not None and not isinstance(graph, str) else ()))
    out.append(tuple(engine.results(all_of_it=True)))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_zero_score_graph_and_null_graph_are_the_unfused_entry(kind):
    sc = lc.random_scenario(4, 9, 12, 1)
    zero = NgramLM.from_ngrams({g: (0.0, 0.0) for g in sc.ngrams}, sc.blank, sc.V, unk=0.0, log10=False)
    assert zero.num_states > 10 and not zero.arc_score.any() and not zero.backoff_score.any() and zero.unk_score == 0
    plain = _trace(sc, kind, None)
    null = _trace(sc, kind, "null")
    fused = _trace(sc, kind, zero)
    assert ds.traces_equal(plain, null)
    assert any((t[2] > 1).any() for t in fused[:-1])  # (the states still move)
    assert ds.traces_equal(plain, [t[:2] for t in fused[:-1]] + [fused[-1]])


@pytest.mark.parametrize("kind", ["timed", "stream_timed"])
def test_timed_twins_report_raw_log_probabilities(kind):
    sc, _, ref, g, engine = _play("flip0", kind)
    hyps, lengths, scores, *rest = engine.results(all_of_it=True)
    frames, logp = (rest[1], rest[2]) if "stream" in kind else (rest[0], rest[1])
    y, s, _ = ref.beams[0][0]
    assert y == (2, 4, 6) and frames[0, 0, :3].tolist() == [0, 1, 2] and (frames[0, 0, 3:] == -1).all()
    raw = [ref.raw[t][(0, 0)] for t in range(3)]  # (the best hypothesis stays in slot 0)
    assert [v for v, _ in raw] == list(y)
    for t, (_, lp) in enumerate(raw):
        assert abs(float(logp[0, 0, t]) - lp) <= 1e-6 * max(1.0, ref.ev.max_lse) + 2.0**-23 * abs(lp), (t, float(logp[0, 0, t]), lp)
    assert float(scores[0, 0]) - float(logp[0, 0, :3].sum()) < -1.0  # the score holds the -1.5 of the LM, the log-probabilities none


@pytest.mark.parametrize("chunk", [1, 3])
def test_a_fused_stream_is_independent_of_its_chunking(chunk):
    sc = lc.random_scenario(4, 9, 12, 1)
    g = lc.build_lm(sc)
    whole = _trace(sc, "stream", g, sc.maxT)
    parts = _trace(sc, "stream", g, chunk)
    offline = _trace(sc, "beam", g)
    assert ds.traces_equal(whole, parts)
    assert ds.traces_equal([t[:3] for t in whole[:-1]] + [whole[-1][:3]], offline)  # ids, states, scores: those of the offline twin


def test_stream_reset_returns_to_state_0_and_a_finished_slot_keeps_its_state():
    V = 9
    grams = {(v,): (-1.0, 0.0) for v in range(1, V)}
    grams.update({(BOS,): (-99.0, -0.25), (BOS, 1): (-0.25, 0.0), (BOS, 1, 2): (-0.25, 0.0), (1, 2): (-0.5, 0.0), (1,): (-1.0, -0.125),
                  (1, 2, 3): (-0.375, 0.0)})
    sc = lc.LmScenario("stream", 0, V, 2, 2, 8, [8, 8], 0, bc.path_script(V, 0, [(1, 2, 3, 4)]), 4, grams)
    g = lc.build_lm(sc)
    q1, q12 = g.walk((1,))[0], g.walk((1, 2))[0]
    assert g.histories[q1] == (BOS, 1) and q1 != g.walk((1,), g.empty_state)[0] and g.histories[q12] == (1, 2)
    eng = LmTwin(sc, "stream", g, chunk=2)
    eng.begin()
    seqs = [()] * 4

    def steps(n):
        nonlocal seqs
        for _ in range(n):
            L = np.stack([sc.script(0, len(seqs[r]), seqs[r]) for r in range(4)])
            p, e, q = eng.step(sc.joint.pred_rows(L))
            seqs = [seqs[a] + ((b,) if b >= 0 else ()) for a, b in zip(p.tolist(), e.tolist())]
        return q.reshape(2, 2)

    eng.feed(2, frames=[2, 2], final=[0, 1])  # slot 1 ends after 1 2
    assert steps(2)[:, 0].tolist() == [q12, q12]
    seqs[0] = seqs[1] = ()
    eng.feed(2, reset=[1, 0], frames=[2, 2], final=[0, 0])  # slot 0 starts again; slot 1 is finished: frozen
    q = steps(1)
    assert q[0, 0] == q1 and q[1, 0] == q12  # (<s> 1, reached from state 0 alone: from E the token 1 leads to the state 1)
    q = steps(1)
    assert q[0, 0] == q12 and q[1, 0] == q12
    hyps, lengths, _ = eng.results()
    assert hyps[:, 0, :2].tolist() == [[1, 2], [1, 2]] and lengths[:, 0].tolist() == [2, 2]


def test_finalisation_with_the_end_of_sentence_score_may_change_the_rank():
    sc, trace, ref, g, engine = _play(lc.finalise_scenario())
    (y0, s0, q0), (y1, s1, q1) = ref.beams[0]
    assert (y0, y1) == ((5, 6), (1, 2)) and float(g.final_score[q0]) == -4.0 and float(g.final_score[q1]) == -0.25 and 0 < s0 - s1 < 3.75
    _, _, scores = engine.results()
    final = g.finalize(torch.from_numpy(scores), torch.from_numpy(trace[-2][2].reshape(1, 2)))
    assert abs(float(final[0, 0]) - (s0 - 4.0)) <= ds.score_bar(2, ref.ev.max_lse, s0) + 2.0**-23 * 4.0
    assert abs(float(final[0, 1]) - (s1 - 0.25)) <= ds.score_bar(2, ref.ev.max_lse, s1) + 2.0**-23 * 0.25
    assert final[0, 1] > final[0, 0]


def test_argument_validation_needs_no_launch():
    sc = lc.flip_scenario(0)
    eng = LmTwin(sc, "beam", None)
    eng.begin()
    g = lc.build_lm(sc).struct(DEV)
    llib = _lib.load_lm()
    args = (eng.rows.data_ptr(), eng.parents.data_ptr(), eng.emitted.data_ptr(), None, None, None) + eng._tail()
    fields = [f for f, _ in _lib.rnntLmGraph._fields_]
    cases = [("num_states", 0), ("num_arcs", -1), ("empty_state", -1), ("empty_state", g.num_states), ("unk_score", math.inf),
             ("unk_score", math.nan)] + [(f, None) for f in fields[4:]]
    for name, value in cases:
        bad = _lib.rnntLmGraph(*[getattr(g, f) for f in fields])
        setattr(bad, name, value)
        assert llib.compute_rnnt_beam_step_lm(*args, ctypes.byref(bad), None) == 2, name
    torch.cuda.synchronize()
    assert (eng.parents.cpu() == -7).all()  # nothing ran


def test_lm_kernels_use_no_scratch():
    import re
    import subprocess
    import tempfile

    import rnnt_speech_recognition_amd as pkg
    from rnnt_speech_recognition_amd.build import LM_LIB_PATH
    from tests.test_isa_audit import READELF, _code_objects

    found = 0
    with tempfile.TemporaryDirectory() as tmp:
        pkg.build()
        for co in _code_objects(LM_LIB_PATH, tmp):  # (the extension library: libwarprnnt.so holds none of them)
            notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True).stdout
            for rec in notes.split(".agpr_count")[1:]:
                name = re.search(r"\.name:\s+(\S+)", rec)
                if name and "lm_kernel" in name.group(1):
                    found += 1
                    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", rec).group(1)) == 0, name.group(1)
    assert found == 5  # three step instantiations, two selects
