"""N-gram LM shallow fusion on the CPU: the builder (lm.NgramLM) against the brute-force back-off recursion, the transition read
back from the arrays, ARPA parsing, the estimator's normalisation, the torch mirror of the fused beam search (joint.BeamJoint /
BeamStreamJoint with lm=) against the float64 restatement of rules 2' and 3' on scripted logits, and the extension interface."""
import itertools
import math

import numpy as np
import pytest
import torch

from rnnt_speech_recognition_amd import joint as jmod
from rnnt_speech_recognition_amd.biasing import ContextGraph
from rnnt_speech_recognition_amd.lm import NgramLM
from tests import decode_scripts as ds
from tests import lm_cases as lc
from tests.lm_cases import BOS, EOS
from tests.test_decode_scripts import _joint_module


# ---- the builder ---------------------------------------------------------------------------------------------------------------
def _check_format(g, V, blank):
    S, A = g.num_states, g.num_arcs
    assert g.arc_offsets.shape == (S + 1,) and g.arc_offsets[0] == 0 and g.arc_offsets[-1] == A
    assert g.arc_tokens.shape == g.arc_next.shape == g.arc_score.shape == (A,)
    assert g.backoff_next.shape == g.backoff_score.shape == g.final_score.shape == (S,)
    assert (g.arc_offsets.dtype, g.arc_tokens.dtype, g.arc_next.dtype, g.arc_score.dtype, g.backoff_next.dtype, g.backoff_score.dtype) == (
        np.int32, np.int32, np.int32, np.float32, np.int32, np.float32)
    for s in range(S):
        tok = g.arc_tokens[g.arc_offsets[s]: g.arc_offsets[s + 1]]
        assert (np.diff(tok) > 0).all() and blank not in tok and ((tok >= 0) & (tok < V)).all()
        cur, hops = s, 0
        while cur != g.empty_state:
            cur, hops = int(g.backoff_next[cur]), hops + 1
        assert hops <= 8
    E = g.empty_state
    assert 0 <= E < S and g.backoff_next[E] == E and ((g.arc_next >= 0) & (g.arc_next < S)).all()
    assert np.isfinite(g.arc_score).all() and np.isfinite(g.backoff_score).all() and np.isfinite(g.unk_score)
    assert g.histories[0] == (BOS,) and g.histories[E] == () and len(set(g.histories)) == S


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_builder_matches_the_brute_force_recursion(order):
    """Random dyadic tables over V = 12: walk() + the </s> score equals the textbook recursion for EVERY sequence of up to 4 tokens
    (exactly: all sums are dyadic); delta equals array_delta and row() on every (s, v); arc_next is the longest-suffix state."""
    V = 12
    rng = np.random.default_rng(100 + order)
    for trial in range(3):
        blank = int(rng.integers(0, V))
        grams = lc.random_ngrams(rng, V, blank, order, bos=trial != 1, eos=trial != 2)
        g = NgramLM.from_ngrams(grams, blank, V, unk=-2.5, log10=False)
        brute = lc.BruteLM(grams, unk=-2.5)
        _check_format(g, V, blank)
        syms = [v for v in range(V) if v != blank]
        checked = 0
        stack = [((), 0, 0.0)]
        while stack:  # every sequence of length <= 4, the state and the score carried along
            y, q, total = stack.pop()
            assert g.histories[q] == next(((BOS,) + y)[k:] for k in range(len(y) + 2) if ((BOS,) + y)[k:] in set(g.histories))
            assert total + float(g.final_score[q]) == brute.sentence(y), (y, total, brute.sentence(y))
            assert total == brute.sentence(y, eos=False)
            checked += 1
            if len(y) < 4:
                for v in syms:
                    nq, beta = g.delta(q, v)
                    stack.append((y + (v,), nq, total + float(beta)))
        assert checked == 1 + 11 + 11**2 + 11**3 + 11**4
        assert g.walk((syms[0], syms[1], syms[0])) [1] == brute.sentence((syms[0], syms[1], syms[0]), eos=False)
        states = set(g.histories)
        for s in range(g.num_states):
            beta, nxt = g.row(s)
            for v in range(V):
                want = lc.array_delta(g, s, v, blank)
                mine = g.delta(s, v)
                assert (mine[0], float(mine[1])) == (want[0], float(want[1])) == (int(nxt[v]), float(beta[v])), (s, v)
            h = g.histories[s]
            for a in range(g.arc_offsets[s], g.arc_offsets[s + 1]):  # arc_next: the longest suffix of h + v that is a state
                seq = h + (int(g.arc_tokens[a]),)
                assert g.histories[g.arc_next[a]] == next(seq[k:] for k in range(len(seq) + 1) if seq[k:] in states)
            if h:
                assert g.histories[g.backoff_next[s]] == next(h[k:] for k in range(1, len(h) + 1) if h[k:] in states)


def test_start_state_and_empty_state_conventions():
    # without <s>: state 0 has no arcs and backs off to E with score 0
    g = NgramLM.from_ngrams({(1,): -1.0, (2,): (-2.0, -0.5), (2, 1): -0.25}, 0, 4, unk=-3.0, log10=False)
    assert g.empty_state == 1 and g.histories[:2] == [(BOS,), ()]
    assert g.arc_offsets[:2].tolist() == [0, 0] and g.backoff_next[0] == 1 and g.backoff_score[0] == 0.0
    assert g.delta(0, 1) == (1, -1.0) and g.delta(0, 2) == (g.histories.index((2,)), -2.0) and g.delta(0, 3) == (1, -3.0)
    assert g.delta(0, 0) == (0, 0.0) and (g.final_score == 0).all()
    # with <s>: state 0 is its history, with arcs and a back-off weight of its own
    g = NgramLM.from_ngrams({(BOS,): (-99.0, -0.75), (1,): -1.0, (BOS, 1): -0.125, (EOS,): -0.5}, 0, 4, unk=-3.0, log10=False)
    assert g.arc_tokens[g.arc_offsets[0]: g.arc_offsets[1]].tolist() == [1] and g.backoff_score[0] == -0.75
    assert g.delta(0, 1) == (1, -0.125) and g.delta(0, 2) == (1, -3.75) and g.delta(1, 2) == (1, -3.0)
    assert g.final_score.tolist() == [-1.25, -0.5]
    assert (NgramLM.from_ngrams({(BOS,): (-99.0, -0.75), (EOS,): -0.5}, 0, 4, log10=False, use_eos=False).final_score == 0).all()


ARPA = """
\\data\\
ngram 1=5
ngram 2=3
ngram 3=1

\\1-grams:
-99 <s> -0.5
-1.0 </s>
-0.25 a -0.75
-0.5 b -0.125
-2.0 <unk>

\\2-grams:
-0.125 <s> a -0.25
-0.375 a b
-0.625 b </s>

\\3-grams:
-0.0625 <s> a b

\\end\\
"""


def test_arpa_parsing_scales_and_rejections(tmp_path):
    ids = {"a": 1, "b": 2}
    g = NgramLM.from_arpa(ARPA, ids, blank=0, vocab_size=4)
    ln10 = math.log(10.0)
    f = lambda x: float(np.float32(x))  # noqa: E731
    assert g.histories == [(BOS,), (), (1,), (2,), (BOS, 1)]
    assert g.arc_offsets.tolist() == [0, 1, 3, 4, 4, 5] and g.arc_tokens.tolist() == [1, 1, 2, 2, 2]
    assert g.arc_next.tolist() == [4, 2, 3, 3, 3]
    assert g.arc_score.tolist() == [f(ln10 * x) for x in (-0.125, -0.25, -0.5, -0.375, -0.0625)]
    assert g.backoff_next.tolist() == [1, 1, 1, 1, 2]
    assert g.backoff_score.tolist() == [f(ln10 * x) for x in (-0.5, 0.0, -0.75, -0.125, -0.25)]
    assert float(g.unk_score) == f(ln10 * -2.0)  # (<unk> in the file wins over unk_log10)
    assert g.final_score[3] == np.float32(ln10 * -0.625) and g.final_score[1] == np.float32(ln10 * -1.0)
    assert g.final_score[2] == np.float32(np.float32(ln10 * -0.75) + np.float32(ln10 * -1.0))
    path = tmp_path / "lm.arpa"
    path.write_text(ARPA)
    h = NgramLM.from_arpa(str(path), ids.get, blank=0, vocab_size=4, scale=0.5, token_bonus=0.25)
    assert h.arc_score.tolist() == [f(0.5 * ln10 * x + 0.25) for x in (-0.125, -0.25, -0.5, -0.375, -0.0625)]
    assert h.backoff_score.tolist() == [f(0.5 * ln10 * x) for x in (-0.5, 0.0, -0.75, -0.125, -0.25)]
    assert float(h.unk_score) == f(0.5 * ln10 * -2.0 + 0.25) and h.final_score[3] == np.float32(0.5 * ln10 * -0.625)
    no_unk = NgramLM.from_arpa(ARPA.replace("-2.0 <unk>\n", ""), ids, blank=0, vocab_size=4, unk_log10=-7.0)
    assert float(no_unk.unk_score) == f(ln10 * -7.0)
    assert (NgramLM.from_arpa(ARPA, ids, blank=0, vocab_size=4, use_eos=False).final_score == 0).all()
    bad = [
        (ARPA, dict(blank=1, vocab_size=4)),                                     # an n-gram holds the blank
        (ARPA, dict(blank=0, vocab_size=2)),                                     # an id outside [0, V)
        (ARPA.replace("-0.375 a b", "-0.375 a <s>"), dict(blank=0, vocab_size=4)),   # <s> anywhere but first
        (ARPA.replace("-0.375 a b", "-0.375 </s> b"), dict(blank=0, vocab_size=4)),  # </s> anywhere but last
        (ARPA.replace("-0.125 <s> a -0.25\n", ""), dict(blank=0, vocab_size=4)),     # <s> a b without its prefix <s> a
        (ARPA.replace("-0.375 a b", "-0.375 a c"), dict(blank=0, vocab_size=4)),     # a word without a token id
    ]
    for text, kw in bad:
        with pytest.raises(ValueError):
            NgramLM.from_arpa(text, ids, **kw)
    with pytest.raises(ValueError):  # order 10: beyond the 8 hops
        NgramLM.from_ngrams({tuple([1] * n): -1.0 for n in range(1, 11)}, 0, 4)
    NgramLM.from_ngrams({tuple([1] * n): -1.0 for n in range(1, 10)}, 0, 4)  # order 9 is taken
    for kw in (dict(scale=math.inf), dict(token_bonus=math.nan), dict(unk=-math.inf)):
        with pytest.raises(ValueError):
            NgramLM.from_ngrams({(1,): -1.0}, 0, 4, **kw)


def test_estimate_is_normalised_in_every_state():
    """Interpolated absolute discounting, order 3, V = 32: sum_v exp(beta(s, v)) + exp(final_score[s]) = 1 within 1e-5 for every
    state (at most 33 stored f32 scores, each rounded to 2^-24 relative; the sums of up to two back-off scores add as much
    again).  It pins the back-off walk: a wrong chain or a wrong sum loses or doubles mass."""
    V, blank = 32, 5
    rng = np.random.default_rng(7)
    syms = [v for v in range(V) if v != blank]
    seqs = [[int(rng.choice(syms[: 4 + n % 27])) for _ in range(int(rng.integers(0, 9)))] for n in range(60)]
    g = NgramLM.estimate(seqs, 3, blank, V, discount=0.6)
    _check_format(g, V, blank)
    assert g.order == 3 and int(g.depth.max()) == 2 and g.arc_offsets[2] - g.arc_offsets[1] == V - 1
    worst = 0.0
    for s in range(g.num_states):
        beta, _ = g.row(s)
        total = sum(math.exp(float(beta[v])) for v in syms) + math.exp(float(g.final_score[s]))
        worst = max(worst, abs(total - 1.0))
    print(f"[estimate] states={g.num_states} arcs={g.num_arcs} worst |sum - 1| = {worst:.3e}")
    assert worst <= 1e-5
    seen = g.walk(seqs[3])[1] + float(g.final_score[g.walk(seqs[3])[0]])
    other = g.score(list(reversed(seqs[3])) + [syms[-1]])
    assert seen > other  # a training sentence outscores a scrambled one
    for kw in (dict(order=0), dict(order=10), dict(discount=0.0), dict(discount=1.0)):
        with pytest.raises(ValueError):
            NgramLM.estimate(seqs, **dict(dict(order=3, blank=blank, vocab_size=V), **kw))
    with pytest.raises(ValueError):
        NgramLM.estimate([[1, blank]], 2, blank, V)


# ---- the torch mirror ----------------------------------------------------------------------------------------------------------
class Mirror:
    """joint.BeamJoint / BeamStreamJoint with lm= on CPU tensors, for lm_cases.run_lm.  Streams: the utterances as slots, one chunk."""

    def __init__(self, sc, g, kind="beam"):
        self.sc, self.kind = sc, kind
        cls = jmod.BeamStreamJoint if "stream" in kind else jmod.BeamJoint
        self.bj = cls(_joint_module(sc.joint, sc.blank), beam=sc.K, token_times="timed" in kind, lm=g)
        assert not self.bj.engine

    def begin(self):
        sc = self.sc
        enc = torch.zeros(sc.B, sc.maxT, 1, dtype=torch.float64)
        if "stream" in self.kind:
            self.bj.begin(sc.B, sc.maxT, sc.maxT)
            self.bj.feed(enc, [min(max(f, 0), sc.maxT) for f in sc.frames], reset=[1] * sc.B, final=[1] * sc.B)
        else:
            self.bj.begin(enc, torch.tensor(sc.frames))

    def step(self, rows):
        with torch.no_grad():
            p, e = self.bj.step(pred_proj=torch.tensor(rows, dtype=torch.float64))
        return p.numpy(), e.numpy(), self.bj.lm_states().numpy()

    def results(self):  # (the beam's own scores: BeamJoint.results() finalises them)
        return tuple(x.numpy() for x in self.bj._torch_results()[:3])


def _play(name, kind="beam"):
    sc = lc.SCENARIOS[name]()
    g = lc.build_lm(sc)
    fn = lambda b, t, y: sc.joint.snap(sc.script(b, t, y))  # noqa: E731
    engine = Mirror(sc, g, kind)
    trace, ref, worst, bar = lc.run_lm(engine, sc.joint, sc.script, g, sc.B, sc.K, sc.frames, sc.maxT, sc.blank, sc.steps, fn,
                                       sc.ties_allowed)
    ds.check_expectations(sc, ref.ev)
    lc.check_scenario(name, sc, ref, g)
    print(f"[{sc.name} {kind}] states={g.num_states} arcs={g.num_arcs} merges={ref.ev.merges} ties={ref.ev.ties} carried={ref.ev.carried} "
          f"min-gap={ref.ev.min_gap:.3g} score-error={worst:.3e} bar={bar:.3e}")
    return sc, trace, ref, g, engine


@pytest.mark.parametrize("kind", ["beam", "timed", "stream", "stream_timed"])
@pytest.mark.parametrize("name", sorted(lc.SCENARIOS))
def test_torch_mirror_against_the_restatement(name, kind):
    _play(name, kind)


def test_offline_results_add_the_end_of_sentence_score_and_are_resorted():
    sc = lc.finalise_scenario()
    g = lc.build_lm(sc)
    engine = Mirror(sc, g)
    fn = lambda b, t, y: sc.joint.snap(sc.script(b, t, y))  # noqa: E731
    _, ref, _, _ = lc.run_lm(engine, sc.joint, sc.script, g, sc.B, sc.K, sc.frames, sc.maxT, sc.blank, sc.steps, fn)
    (y0, s0, q0), (y1, s1, q1) = ref.beams[0]
    assert (y0, y1) == ((5, 6), (1, 2)) and float(g.final_score[q0]) == -4.0 and float(g.final_score[q1]) == -0.25
    assert 0 < s0 - s1 < 3.75
    hyps, lengths, scores = engine.bj.results()
    assert hyps[0, :, :2].tolist() == [[1, 2], [5, 6]] and lengths[0].tolist() == [2, 2]
    assert abs(float(scores[0, 0]) - (s1 - 0.25)) < 1e-6 and abs(float(scores[0, 1]) - (s0 - 4.0)) < 1e-6


@pytest.mark.parametrize("kind", ["beam", "timed", "stream", "stream_timed"])
def test_an_all_zero_lm_is_the_unfused_search(kind):
    sc = lc.random_scenario(4, 9, 12, 1)
    zero = NgramLM.from_ngrams({(v,): (0.0, 0.0) for v in range(1, sc.V)}, sc.blank, sc.V, unk=0.0, log10=False)
    assert not zero.arc_score.any() and not zero.backoff_score.any() and zero.unk_score == 0 and not zero.final_score.any()

    def run(lm):
        eng = Mirror(sc, lm, kind)
        eng.begin()
        seqs, out = [()] * (sc.B * sc.K), []
        for step in range(sc.steps):
            L = np.stack([sc.script(r // sc.K, step, seqs[r]) for r in range(sc.B * sc.K)])
            p, e, _ = eng.step(sc.joint.pred_rows(L))
            seqs = [seqs[a] + ((b,) if b >= 0 else ()) for a, b in zip(p.tolist(), e.tolist())]
            out.append((p.copy(), e.copy()))
        out.append(tuple(x.numpy() for x in eng.bj.results()))
        return out

    assert ds.traces_equal(run(None), run(zero))


def test_argument_validation():
    jl = jmod.JointLoss(1, 64, 9)
    lm9 = NgramLM.from_ngrams({(1,): -1.0}, 0, 9)
    ctx = ContextGraph([(1, 2)], blank=0, vocab_size=9)
    jmod.BeamJoint(jl, beam=2, lm=lm9)
    for cls in (jmod.BeamJoint, jmod.BeamStreamJoint):
        with pytest.raises(ValueError):
            cls(jl, beam=2, lm=lm9, context=ctx)  # one state word per hypothesis
        with pytest.raises(ValueError):
            cls(jl, beam=2, lm=NgramLM.from_ngrams({(1,): -1.0}, 0, 8))  # built for another vocabulary
        with pytest.raises(ValueError):
            cls(jl, beam=2, lm=NgramLM.from_ngrams({(1,): -1.0}, 3, 9))  # built for another blank
    for kw in (dict(blank=9, vocab_size=9), dict(blank=0, vocab_size=0)):
        with pytest.raises(ValueError):
            NgramLM.from_ngrams({(1,): -1.0}, **kw)
    for grams in ({(): -1.0}, {(0,): -1.0}, {(9,): -1.0}, {(-1,): -1.0}, {(1, BOS): -1.0, (1,): -1.0}, {(EOS, 1): -1.0, (EOS,): -1.0},
                  {(1, 2): -1.0}, {(1,): math.nan}, {(1,): (-1.0, math.inf)}, {("a",): -1.0}):
        with pytest.raises(ValueError):
            NgramLM.from_ngrams(grams, 0, 9)


# ---- the extension interface -----------------------------------------------------------------------------------------------------
def test_extension_header_binding_and_exports_agree():
    """include/rnnt_lm.h declares the four LM steps and libwarprnnt_lm.so exports them and nothing else of the interface; each
    twin's signature is its base step's plus two; the base and bias libraries hold nothing of it."""
    import ctypes
    import os
    import re
    import shutil
    import subprocess

    import rnnt_speech_recognition_amd as pkg
    from rnnt_speech_recognition_amd import _lib
    from rnnt_speech_recognition_amd.build import BIAS_LIB_PATH, LM_LIB_PATH

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def declared(name):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", name)).read(), flags=re.S)
        return {m.group(1): m.group(2) for m in re.finditer(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(([^;{]*)\)\s*;", text)}

    ext, base = declared("rnnt_lm.h"), declared("rnnt.h")
    assert sorted(ext) == sorted(_lib.LM_SYMBOLS) and len(ext) == 4 and not set(ext) & set(base)
    pkg.build()
    lib, llib = _lib.load(), _lib.load_lm()
    strip = lambda s: re.sub(r"\s+", " ", s).strip()  # noqa: E731
    for name in ext:
        assert not hasattr(lib, name), name
        fn, twin = getattr(llib, name), getattr(lib, name[: -len("_lm")])
        assert ctypes.cast(fn, ctypes.c_void_p).value and fn.restype is ctypes.c_int
        assert list(fn.argtypes[:-2]) == list(twin.argtypes) and fn.argtypes[-1] is ctypes.c_void_p
        assert strip(ext[name]).startswith(strip(base[name[: -len("_lm")]])), name
        assert strip(ext[name]).endswith("const rnntLmGraph *graph, int *lm_states"), name
    header = open(os.path.join(root, "include", "rnnt_lm.h")).read()
    fields = re.findall(r"^\s+(?:const\s+)?(?:int|float)\s+\*?(\w+);", header[header.index("typedef struct"):], flags=re.M)
    assert fields == [f for f, _ in _lib.rnntLmGraph._fields_] and len(fields) == 10
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("binutils nm not available")

    def exported(path):
        out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return [ln.split()[-1] for ln in out.splitlines() if ln.strip()]

    names = exported(LM_LIB_PATH)
    assert sorted(n for n in names if not n.startswith("_Z") and not n.startswith("__hip_cuid_")) == sorted(_lib.LM_SYMBOLS)
    assert all(n.startswith("_ZN4rnnt") and "kernel" in n for n in names if n.startswith("_Z"))
    assert not [n for n in exported(_lib.LIB_PATH) + exported(BIAS_LIB_PATH) if "_lm" in n.lower().replace("_lma", "")]


def test_extension_argument_validation_needs_no_device():
    import ctypes

    import rnnt_speech_recognition_amd as pkg
    from rnnt_speech_recognition_amd import _lib

    pkg.build()
    llib = _lib.load_lm()
    fake = ctypes.c_void_p(256)
    o = _lib.make_options(0, 0, 10, 1)
    step = lambda g, states=None: llib.compute_rnnt_beam_step_lm(fake, fake, fake, None, None, None, 64, 28, 2, 4, 0, fake, o, g, states)  # noqa: E731
    G = _lib.rnntLmGraph
    ok = [3, 2, 1, -1.0, 256, 256, 256, 256, 256, 256]
    for k, v in ((0, 0), (1, -1), (2, -1), (2, 3), (3, math.inf), (3, -math.inf), (3, math.nan), (8, None), (9, None),
                 (4, None), (5, None), (6, None), (7, None)):
        bad = list(ok)
        bad[k] = v
        assert step(ctypes.byref(G(*bad))) == 2, (k, v)
    assert step(ctypes.byref(G(*ok)), ctypes.c_void_p(258)) == 2  # misaligned lm_states
    assert llib.compute_rnnt_beam_step_lm(None, fake, fake, None, None, None, 64, 28, 2, 4, 0, fake, o, None, None) == 2  # NULL graph: the base step's checks


def test_the_beam_translation_units_set_the_same_constants():
    import os
    import re

    csrc = os.path.join(os.path.dirname(ds.BEAM_SOURCE))
    found = []
    for name in ("beam_kernels.hip", "beam_lm_kernels.hip"):
        text = open(os.path.join(csrc, name)).read()
        found.append((re.search(r"kBeamMax\s*=\s*(\d+)", text).group(1), re.search(r"kHashMul\s*=\s*(0x[0-9A-Fa-f]+)", text).group(1)))
    assert found[0] == found[1] and int(found[0][1], 16) == ds.hash_multiplier()
    from rnnt_speech_recognition_amd import lm as lm_mod

    header = open(os.path.join(ds.ROOT, "include", "rnnt_lm.h")).read()
    assert int(re.search(r"#define RNNT_LM_MAX_HOPS (\d+)", header).group(1)) == lm_mod.MAX_HOPS == 8
