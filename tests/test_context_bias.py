"""Contextual biasing on the CPU: the context-graph builder (biasing.ContextGraph) against the brute-force restatement of its
scoring model, the transition read back from the uploaded arrays, the torch mirror of the biased beam search (joint.BeamJoint with
context=) against the float64 restatement of rules 2' and 3' on scripted logits, finalisation, and argument validation."""
import math

import numpy as np
import pytest
import torch

from rnnt_speech_recognition_amd import joint as jmod
from rnnt_speech_recognition_amd.biasing import ContextGraph
from tests import bias_cases as bc
from tests import decode_scripts as ds
from tests.test_decode_scripts import _joint_module


# ---- the builder ---------------------------------------------------------------------------------------------------------------
def _check_graph(phrases, boosts, V, blank):
    g = ContextGraph(phrases, boost=boosts, blank=blank, vocab_size=V)
    brute = bc.BruteGraph(phrases, boosts, blank)
    S, A = g.num_states, g.num_arcs
    assert S == len(brute.nodes) and g.arc_offsets.shape == (S + 1,) and g.arc_offsets[0] == 0 and g.arc_offsets[-1] == A
    assert g.arc_tokens.shape == g.arc_next.shape == g.arc_bias.shape == (A,) and g.fail_bias.shape == (S,)
    assert (g.arc_offsets.dtype, g.arc_tokens.dtype, g.arc_next.dtype, g.arc_bias.dtype, g.fail_bias.dtype) == (
        np.int32, np.int32, np.int32, np.float32, np.float32)
    for s in range(S):  # the format of include/rnnt_bias.h
        tok = g.arc_tokens[g.arc_offsets[s]: g.arc_offsets[s + 1]]
        assert (np.diff(tok) > 0).all() and blank not in tok and ((tok >= 0) & (tok < V)).all()
    assert ((g.arc_next >= 0) & (g.arc_next < S)).all() and np.isfinite(g.arc_bias).all()
    assert np.isfinite(g.fail_bias).all() and (g.fail_bias <= 0).all() and g.fail_bias[0] == 0
    # state <-> node: walk every node's path from the root
    state = {(): 0}
    for n in sorted(brute.nodes, key=len):
        if n:
            state[n], b = bc.array_delta(g, state[n[:-1]], n[-1], blank)
            assert float(b) == brute.gain(n) - brute.gain(n[:-1])
    assert sorted(state.values()) == list(range(S))
    for n, s in state.items():  # delta for every (state, token), three ways
        assert float(g.fail_bias[s]) == -brute.pending(n)
        for v in range(V):
            want_n, want_b = brute.delta(n, v)
            got = bc.array_delta(g, s, v, blank)
            assert (got[0], float(got[1])) == (state[want_n], want_b), (n, v)
            mine = g.delta(s, v)
            assert (mine[0], float(mine[1])) == (got[0], float(got[1]))
        beta, nxt = g.row(s)
        assert beta.tolist() == [float(bc.array_delta(g, s, v, blank)[1]) for v in range(V)]
        assert nxt.tolist() == [bc.array_delta(g, s, v, blank)[0] for v in range(V)]
    return g


def test_builder_matches_the_brute_force_restatement_on_200_random_phrase_sets():
    rng = np.random.default_rng(2024)
    seen = dict(prefix=0, suffix=0, infix=0)
    for _ in range(200):
        V = int(rng.integers(8, 65))
        blank = int(rng.integers(0, V))
        phrases, boosts = bc.random_phrases(rng, V, blank, int(rng.integers(1, 41)))
        assert all(1 <= len(p) <= 6 for p in phrases)
        ps = set(phrases)
        seen["prefix"] += any(p != q and q[: len(p)] == p for p in ps for q in ps)
        seen["suffix"] += any(p != q and len(q) > len(p) and q[len(q) - len(p):] == p for p in ps for q in ps)
        seen["infix"] += any(p != q and any(q[i: i + len(p)] == p for i in range(1, len(q) - len(p))) for p in ps for q in ps)
        _check_graph(phrases, boosts, V, blank)
    assert min(seen.values()) >= 50, seen


def test_overlap_and_prefix_by_hand():
    g = _check_graph([(1, 2, 3), (2, 3, 4)], [1.0, 0.5], 8, 0)
    q, total = g.walk([1, 2, 3, 4])
    assert total == 4.5 and float(g.fail_bias[q]) == 0.0  # (1, 2, 3) banks 3.0; the move to (2, 3, 4) pays its gain, 1.5
    g = _check_graph([(1, 2), (1, 2, 3, 4)], [1.5, 0.25], 8, 0)
    q, total = g.walk([1, 2, 3])
    assert total == 3.25 and float(g.fail_bias[q]) == -0.25  # (1, 2) is kept, the boost of 3 is pending
    q, total = g.walk([1, 2, 3, 7])
    assert (q, total) == (0, 3.0)
    # a phrase completed only as a proper suffix of a longer live match is not banked (documented in biasing.py)
    g = _check_graph([(1, 2, 3, 5), (2, 3)], [1.0, 1.0], 8, 0)
    assert g.walk([1, 2, 3, 7]) == (0, 0.0) and g.walk([2, 3, 7]) == (0, 2.0)


def test_root_only_graph():
    g = ContextGraph([], blank=0, vocab_size=5)
    assert (g.num_states, g.num_arcs, g.arc_offsets.tolist(), g.fail_bias.tolist()) == (1, 0, [0, 0], [0.0])
    assert g.delta(0, 3) == (0, 0.0)


def test_argument_validation():
    ok = dict(blank=0, vocab_size=8)
    for phrases, kw in (([()], ok), ([(1, 0)], ok), ([(8,)], ok), ([(-1,)], ok), ([(1,)], dict(ok, boost=0.0)),
                        ([(1,)], dict(ok, boost=-1.0)), ([(1,)], dict(ok, boost=math.inf)), ([(1,)], dict(ok, boost=math.nan)),
                        ([(1,), (2,)], dict(ok, boost=[1.0])), ([(1,)], dict(blank=8, vocab_size=8)), ([(1,)], dict(blank=0))):
        with pytest.raises(ValueError):
            ContextGraph(phrases, **kw)
    g = ContextGraph.from_texts(["ab", "b"], lambda t: [ord(c) - 96 for c in t], boost=[2.0, 0.5], **ok)
    assert g.phrases == [(1, 2), (2,)]
    jl = jmod.JointLoss(1, 64, 9)
    with pytest.raises(ValueError):
        jmod.BeamJoint(jl, beam=2, context=g)  # built for another vocabulary


# ---- the torch mirror ----------------------------------------------------------------------------------------------------------
class MirrorBiased:
    def __init__(self, sc, g):
        self.sc = sc
        self.bj = jmod.BeamJoint(_joint_module(sc.joint, sc.blank), beam=sc.K, context=g)
        assert not self.bj.engine

    def begin(self):
        self.bj.begin(torch.zeros(self.sc.B, self.sc.maxT, 1, dtype=torch.float64), torch.tensor(self.sc.frames))

    def step(self, rows):
        with torch.no_grad():
            p, e = self.bj.step(pred_proj=torch.tensor(rows, dtype=torch.float64))
        return p.numpy(), e.numpy(), self.bj.bias_states().numpy()

    def results(self):  # (the beam's own scores: BeamJoint.results() finalises them)
        return tuple(x.numpy() for x in self.bj._torch_results())


def _play(sc, engine_of=MirrorBiased):
    g = bc.build_graph(sc)
    fn = lambda b, t, y: sc.joint.snap(sc.script(b, t, y))  # noqa: E731
    engine = engine_of(sc, g)
    trace, ref, worst, bar = bc.run_biased(engine, sc.joint, sc.script, g, sc.B, sc.K, sc.frames, sc.maxT, sc.blank, sc.steps, fn,
                                           sc.ties_allowed)
    ds.check_expectations(sc, ref.ev)
    print(f"[{sc.name}] states={g.num_states} arcs={g.num_arcs} merges={ref.ev.merges} ties={ref.ev.ties} carried={ref.ev.carried} "
          f"min-gap={ref.ev.min_gap:.3g} score-error={worst:.3e} bar={bar:.3e}")
    return trace, ref, g, engine


def _unbiased_best(sc):
    ref = ds.BeamRestatement(lambda b, t, y: sc.joint.snap(sc.script(b, t, y)), sc.B, sc.K, sc.frames, sc.maxT, sc.blank)
    for _ in range(sc.steps):
        ref.step()
    return [beam[0] for beam in ref.beams]


@pytest.mark.parametrize("dtype", [0, 1])
def test_a_boost_flips_the_winner(dtype):
    sc = bc.flip_scenario(dtype)
    _, ref, _, _ = _play(sc)
    assert [y for y, _ in _unbiased_best(sc)] == [(1, 3, 5), (1, 3, 5)]
    assert [beam[0][0] for beam in ref.beams] == [(2, 4, 6), (2, 4, 6)]


@pytest.mark.parametrize("dtype", [0, 1])
def test_a_broken_match_gives_the_bonus_back_exactly(dtype):
    sc = bc.takeback_scenario(dtype)
    trace, ref, g, _ = _play(sc)
    y, s, q = ref.beams[0][0]
    (y0, s0), = _unbiased_best(sc)
    assert y == y0 == (1, 2, 7) and q == 0 and g.walk(y) == (0, 0.0)
    # +0.5 +0.5 -1.0 = 0 exactly; the scores still differ by the mass of the merged-in blank routes (e^-6.5 each), which the
    # bonus re-weights while it is held
    assert abs(s - s0) < 1e-2
    assert [t[2][0] for t in trace[:3]] == [g.walk([1])[0], g.walk([1, 2])[0], 0]


@pytest.mark.parametrize("dtype", [0, 1])
def test_overlapping_phrases_move_along_the_merged_fail_arc(dtype):
    sc = bc.overlap_scenario(dtype)
    trace, ref, g, _ = _play(sc)
    y, s, q = ref.beams[0][0]
    (y0, s0), = _unbiased_best(sc)
    assert y == y0 == (1, 2, 3, 4) and q == g.walk((2, 3, 4))[0] != 0
    assert g.walk(y)[1] == 4.5 and abs((s - s0) - 4.5) < 1e-2  # 3 x 1.0 banked at (1, 2, 3), then gain(2, 3, 4) = 1.5


@pytest.mark.parametrize("dtype", [0, 1])
def test_a_phrase_that_is_a_prefix_of_another_is_kept(dtype):
    sc = bc.prefix_scenario(dtype)
    _, ref, g, _ = _play(sc)
    y, s, q = ref.beams[0][0]
    (y0, s0), = _unbiased_best(sc)
    assert y == y0 == (1, 2, 3, 7) and q == 0 and g.walk(y)[1] == 3.0 and abs((s - s0) - 3.0) < 1e-2


@pytest.mark.parametrize("K", [2, 5])
def test_declared_key_and_candidate_ties(K):
    _play(bc.tie_scenario(K))


@pytest.mark.parametrize("K", [3, 4])
def test_merges_keep_one_state(K):
    _play(bc.merge_scenario(K))


@pytest.mark.parametrize("K,B,seed,dtype", [(1, 3, 11, 0), (4, 9, 12, 1), (16, 5, 13, 0)])
def test_random_scripts_under_random_phrases(K, B, seed, dtype):
    _play(bc.random_scenario(K, B, seed, dtype))


def test_a_nan_row_takes_no_part():
    _play(bc.random_scenario(3, 4, 14, 0, nan_at=(2, 3)))


def test_offline_results_are_finalised_and_resorted():
    """Two hypotheses: 1 2 (mid-phrase of (1, 2, 3): 4.0 pending) ends 3.25 ahead of the model's favourite 5 6, and falls behind it."""
    V = 9
    sc = bc.BiasScenario("finalise", 0, V, 1, 2, 2, [2], 0, bc.path_script(V, 0, [(5, 6), (1, 2)]), 2, [(1, 2, 3)], [2.0])
    _, ref, g, engine = _play(sc)
    (y0, s0, q0), (y1, s1, q1) = ref.beams[0]
    assert (y0, y1) == ((1, 2), (5, 6)) and q0 == g.walk((1, 2))[0] and q1 == 0 and float(g.fail_bias[q0]) == -4.0
    assert 0 < s0 - s1 < 4.0
    hyps, lengths, scores = engine.bj.results()
    assert hyps[0, :, :2].tolist() == [[5, 6], [1, 2]] and lengths[0].tolist() == [2, 2]
    assert abs(float(scores[0, 0]) - s1) < 1e-6 and abs(float(scores[0, 1]) - (s0 - 4.0)) < 1e-6  # (the restatement reads f32 logits)


def test_stream_mirror_reset_returns_to_the_root_and_finished_slots_keep_their_state():
    V = 9
    sc = bc.BiasScenario("stream", 0, V, 2, 2, 4, [4, 4], 0, bc.path_script(V, 0, [(1, 2, 3, 4)]), 4, [(1, 2, 3, 4)], [0.5])
    g = bc.build_graph(sc)
    bj = jmod.BeamStreamJoint(_joint_module(sc.joint, 0), beam=2, context=g)
    bj.begin(2, 2, 8)
    enc = torch.zeros(2, 2, 1, dtype=torch.float64)
    seqs = [()] * 4

    def steps(n, t0):
        nonlocal seqs
        for t in range(t0, t0 + n):
            L = np.stack([sc.script(0, len(seqs[r]), seqs[r]) for r in range(4)])
            p, e = bj.step(pred_proj=torch.tensor(sc.joint.pred_rows(L), dtype=torch.float64))
            seqs = [seqs[a] + ((b,) if b >= 0 else ()) for a, b in zip(p.tolist(), e.tolist())]

    bj.feed(None, [0, 0], reset=[1, 1])
    bj.feed(enc, [2, 2], final=[0, 1])  # slot 1 ends mid-phrase
    steps(2, 0)
    q12 = g.walk((1, 2))[0]
    assert bj.bias_states().reshape(2, 2)[:, 0].tolist() == [q12, q12]
    seqs[0] = seqs[1] = ()
    bj.feed(enc, [2, 2], reset=[1, 0])  # slot 0 starts again; slot 1 is finished: frozen
    assert bj._states[0] == [0]
    steps(2, 0)
    st = bj.bias_states().reshape(2, 2)
    assert st[0, 0] == q12 and st[1, 0] == q12 and bj.results()[1][:, 0].tolist() == [2, 2]


# ---- the extension interface -----------------------------------------------------------------------------------------------------
def test_extension_header_binding_and_exports_agree():
    """include/rnnt_bias.h declares the four biased steps and libwarprnnt_bias.so defines them; include/rnnt.h and libwarprnnt.so
    are unchanged; each twin's signature is its base step's plus two."""
    import ctypes
    import os
    import re
    import rnnt_speech_recognition_amd as pkg
    from rnnt_speech_recognition_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def declared(name):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", name)).read(), flags=re.S)
        return {m.group(1): m.group(2) for m in re.finditer(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(([^;{]*)\)\s*;", text)}

    ext, base = declared("rnnt_bias.h"), declared("rnnt.h")
    assert sorted(ext) == sorted(_lib.BIAS_SYMBOLS) and len(ext) == 4 and not set(ext) & set(base)
    pkg.build()
    lib, blib = _lib.load(), _lib.load_bias()
    strip = lambda s: re.sub(r"\s+", " ", s).strip()  # noqa: E731
    for name in ext:
        assert not hasattr(lib, name), name  # the base library is what it was
        fn, twin = getattr(blib, name), getattr(lib, name[: -len("_biased")])
        assert ctypes.cast(fn, ctypes.c_void_p).value and fn.restype is ctypes.c_int
        assert list(fn.argtypes[:-2]) == list(twin.argtypes) and fn.argtypes[-1] is ctypes.c_void_p
        assert strip(ext[name]).startswith(strip(base[name[: -len("_biased")]])), name
        assert strip(ext[name]).endswith("const rnntBiasGraph *graph, int *bias_states"), name


def test_extension_library_exports_the_four_steps_and_nothing_else_of_the_interface():
    """libwarprnnt_bias.so exports the biased steps alone (csrc/rnnt_bias.map): no base entry point is defined twice in a process
    that links both libraries, and libwarprnnt.so holds nothing of the extension."""
    import shutil
    import subprocess

    import rnnt_speech_recognition_amd as pkg
    from rnnt_speech_recognition_amd import _lib
    from rnnt_speech_recognition_amd.build import BIAS_LIB_PATH

    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("binutils nm not available")
    pkg.build()

    def exported(path):
        out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return [ln.split()[-1] for ln in out.splitlines() if ln.strip()]

    names = exported(BIAS_LIB_PATH)
    assert sorted(n for n in names if not n.startswith("_Z") and not n.startswith("__hip_cuid_")) == sorted(_lib.BIAS_SYMBOLS)
    assert all(n.startswith("_ZN4rnnt") and "kernel" in n for n in names if n.startswith("_Z"))
    assert not [n for n in exported(_lib.LIB_PATH) if "bias" in n.lower()]


def test_extension_argument_validation_needs_no_device():
    import ctypes

    import rnnt_speech_recognition_amd as pkg
    from rnnt_speech_recognition_amd import _lib

    pkg.build()
    blib = _lib.load_bias()
    fake = ctypes.c_void_p(256)
    o = _lib.make_options(0, 0, 10, 1)
    step = lambda g, states=None: blib.compute_rnnt_beam_step_biased(fake, fake, fake, None, None, None, 64, 28, 2, 4, 0, fake, o, g, states)  # noqa: E731
    G = _lib.rnntBiasGraph
    assert step(ctypes.byref(G(0, 0, 256, 256, 256, 256, 256))) == 2   # S < 1
    assert step(ctypes.byref(G(1, -1, 256, 256, 256, 256, 256))) == 2  # A < 0
    for k in range(5):  # a NULL array with A > 0
        ptrs = [256] * 5
        ptrs[k] = None
        assert step(ctypes.byref(G(3, 2, *ptrs))) == 2, k
    assert step(ctypes.byref(G(3, 2, 256, 256, 256, 256, 256)), ctypes.c_void_p(258)) == 2  # misaligned bias_states
    assert blib.compute_rnnt_beam_step_biased(None, fake, fake, None, None, None, 64, 28, 2, 4, 0, fake, o, None, None) == 2  # NULL graph: the base step's checks


# ---- the decoders' context= on the torch route ---------------------------------------------------------------------------------
def _model_logits(model, enc):
    def fn(b, t, y):
        with torch.no_grad():
            g = model.prediction(torch.tensor([(0,) + tuple(y)]))[:, -1:, :]
            return model.joint.logits(enc[b: b + 1, t: t + 1], g)[0, 0, 0].double().numpy()
    return fn


@pytest.mark.parametrize("K", [1, 4])
def test_beam_search_batch_with_a_context_against_the_restatement(K):
    """decoding.beam_search_batch / beam_decode_batch(context=) on CPU tensors (the torch mirror): the beams of the restatement,
    finalised and stably re-sorted here by hand; with token_times the frames and log-probabilities follow their hypotheses."""
    import rnnt_speech_recognition_amd as pkg
    from rnnt_speech_recognition_amd import decoding
    from tests.test_frontend import small_model

    model = small_model(0).double().eval()
    with torch.no_grad():
        model.joint.b2[0] += 0.5
    torch.manual_seed(200)
    B = 4
    mel = torch.randn(B, 20, 8, dtype=torch.float64)
    spec_lengths = torch.tensor([20, 13, 0, 7])
    rng = np.random.default_rng(3)
    phrases, boosts = bc.random_phrases(rng, 12, 0, 10, max_len=3)
    g = ContextGraph(phrases, boost=boosts, blank=0, vocab_size=12)
    with torch.no_grad():
        enc = model.encoder(mel)
    frames = pkg.reduced_lengths(spec_lengths, model.hp.time_reduction_factor)
    T = enc.shape[1]
    ref = bc.BiasedBeamRestatement(_model_logits(model, enc), g, B, K, frames.tolist(), T, 0)
    for _ in range(T):
        ref.step()
    with torch.no_grad():
        plain = decoding.beam_search_batch(model, enc, frames, beam=K)
        ids, lengths, scores, fr, logp = decoding.beam_search_batch(model, enc, frames, beam=K, token_times=True, context=g)
        untimed = decoding.beam_search_batch(model, enc, frames, beam=K, context=g)
        best = decoding.beam_decode_batch(model, mel, spec_lengths, beam=K, context=g)
    assert all(torch.equal(a, b) for a, b in zip(untimed, (ids, lengths, scores)))
    assert torch.equal(best[0], ids[:, 0]) and torch.equal(best[2], scores[:, 0])
    moved = reranked = 0
    for b in range(B):
        final = [(y, s + float(g.fail_bias[q]), q) for y, s, q in ref.beams[b]]
        order = sorted(range(len(final)), key=lambda k: -final[k][1])  # (stable)
        reranked += order != list(range(len(final)))
        for k, j in enumerate(order):
            y, s, q = final[j]
            n = int(lengths[b, k])
            assert ids[b, k, :n].tolist() == list(y) and not ids[b, k, n:].any(), (b, k)
            assert abs(float(scores[b, k]) - s) <= 1e-5 * max(1.0, abs(s)), (b, k, float(scores[b, k]), s)
            row = fr[b, k, :n].tolist()
            assert row == sorted(set(row)) and (fr[b, k, n:] == -1).all() and (logp[b, k, :n] <= 0).all() and not logp[b, k, n:].any()
            if K == 1:  # no merges: the score is the log-probabilities, the blanks' included, plus the bias that was kept
                assert float(scores[b, k]) <= float(logp[b, k].sum()) + g.walk(y)[1] + float(g.fail_bias[q]) + 1e-9
        for k in range(len(final), K):
            assert int(lengths[b, k]) == 0 and float(scores[b, k]) == -math.inf
        moved += ids[b, 0].tolist() != plain[0][b, 0].tolist()
    assert moved > 0, "the context changes no best hypothesis: the case shows nothing"
    if K > 1:
        assert reranked > 0, "finalisation changes no order: the case shows nothing"


def test_both_beam_translation_units_set_the_same_constants():
    import os
    import re

    csrc = os.path.join(os.path.dirname(ds.BEAM_SOURCE))
    found = []
    for name in ("beam_kernels.hip", "beam_bias_kernels.hip"):
        text = open(os.path.join(csrc, name)).read()
        found.append((re.search(r"kBeamMax\s*=\s*(\d+)", text).group(1), re.search(r"kHashMul\s*=\s*(0x[0-9A-Fa-f]+)", text).group(1)))
    assert found[0] == found[1] and int(found[0][1], 16) == ds.hash_multiplier()
