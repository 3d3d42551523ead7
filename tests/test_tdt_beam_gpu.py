"""Batched TDT beam search on an MI355X, through the C ABI (compute_rnnt_tdt_beam_*) and through tdt.TDTBeamJoint, against the float64
restatement of include/rnnt_tdt_beam.h (tests/tdt_beam_cases.py, brute force over all V D candidates) fed with the f32 logits
compute_rnnt_joint_logits returns for each hypothesis alone at alphabet_size = V + D.  ids, lengths, cursors, parents, emitted,
frames and durations are compared exactly at every step and nothing is skipped; scores within decode_scripts.score_bar(2 n, ...).
The gap precondition (adjacent deciding candidates tied exactly or more than twice the bar apart) is asserted on the restatement
alone; the random models take the first seed of a fixed list on which it holds.  Each test prints the events it rests on."""
import math

import numpy as np
import pytest
import torch

from rnnt_speech_recognition_amd import _lib, tdt
from rnnt_speech_recognition_amd import joint as jmod
from tests import tdt_beam_cases as bc
from tests import tdt_decode_cases as tc
from tests.test_tdt_greedy import small_tdt_model
from tests.test_tdt_greedy_gpu import DeviceJoint, LogitsEntry, _dev, _opts, random_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
D1, D5, D8 = [1], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4, 5, 6, 8]

# (V, D) -> (joint_dtype, J): test_tdt_greedy_gpu.SPLITS, restated -- where the duration head lies among the chunks and slices
SPLITS = {
    (2, 1): (0, 64),        # R = 3
    (27, 5): (0, 64),       # R = 32 exactly: one chunk
    (30, 5): (0, 64),       # the head straddles two chunks of one slice
    (32, 5): (1, 128),      # the head starts a chunk
    (128, 1): (1, 128),     # the head starts a chunk and a slice
    (126, 5): (1, 640),     # the head straddles a slice boundary: two workgroups write a row's duration logits
    (125, 8): (1, 128),     # eight durations across the slice boundary
    (1030, 5): (1, 128),    # 33 chunks, 9 slices
}


class AbiBeam:
    """The caller of the C ABI.  timed: the {frame, duration} rows; diag: the four diagnostics arrays; ws: a workspace to use."""

    def __init__(self, sc, poison=False, timed=True, diag=False, stream=None, ws=None):
        c = self.case = sc.case
        self.K, self.timed, self.stream = sc.K, timed, stream
        self.W2, self.b2, self.enc = _dev(c.W2), _dev(c.b2), _dev(c.enc_proj)
        self.frames = _dev(np.asarray(c.frames, np.int32))
        nbytes = _lib.tdt_beam_workspace_bytes(c.maxT, c.B, sc.K, c.J, c.V, c.D, c.dtype, timed)
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV) if ws is None else ws
        assert self.ws.numel() >= nbytes and self.ws.data_ptr() % 256 == 0
        if poison:
            self.ws.fill_(0xFF)
        R = c.B * sc.K
        self.parents = torch.full((R,), -7, dtype=torch.int32, device=DEV)
        self.emitted = torch.full((R,), -7, dtype=torch.int32, device=DEV)
        self.rows = torch.empty(R, c.J, device=DEV)
        self.diag = None
        if diag:
            self.diag = (torch.full((R, sc.K), float("nan"), device=DEV), torch.full((R, sc.K), -7, dtype=torch.int32, device=DEV),
                         torch.full((R, c.D), float("nan"), device=DEV), torch.full((R, 2), float("nan"), device=DEV))
        self.dur = (_lib.ctypes.c_int * c.D)(*c.durations)
        self.lib = _lib.load_tdtbeam()

    def _tail(self):
        c = self.case
        return (c.J, c.V, c.D, c.B, self.K, c.dtype, int(self.timed), self.ws.data_ptr(), _opts(c.blank, c.maxT, self.stream))

    def begin(self):
        c = self.case
        torch.cuda.synchronize()  # (a side stream: the buffers above were filled on the current one)
        _lib.check(self.lib.compute_rnnt_tdt_beam_begin(self.enc.data_ptr(), self.frames.data_ptr(), self.W2.data_ptr(), self.b2.data_ptr(),
                                                        c.J, c.V, self.dur, *self._tail()[2:]), "compute_rnnt_tdt_beam_begin")

    def step(self, rows):
        self.rows.copy_(torch.from_numpy(rows))
        torch.cuda.synchronize()
        d = [None] * 4 if self.diag is None else [x.data_ptr() for x in self.diag]
        _lib.check(self.lib.compute_rnnt_tdt_beam_step(self.rows.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(), *d,
                                                       *self._tail()), "compute_rnnt_tdt_beam_step")
        torch.cuda.synchronize()
        return self.parents.cpu().numpy(), self.emitted.cpu().numpy()

    def results(self):
        c, K = self.case, self.K
        hyps = torch.full((c.B, K, c.maxT), -7, dtype=torch.int32, device=DEV)
        lengths = torch.full((c.B, K), -7, dtype=torch.int32, device=DEV)
        scores = torch.full((c.B, K), float("nan"), device=DEV)
        cursors = torch.full((c.B, K), -7, dtype=torch.int32, device=DEV)
        fr = torch.full((c.B, K, c.maxT), -7, dtype=torch.int32, device=DEV) if self.timed else None
        du = torch.full((c.B, K, c.maxT), -7, dtype=torch.int32, device=DEV) if self.timed else None
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        torch.cuda.synchronize()
        _lib.check(self.lib.compute_rnnt_tdt_beam_results(hyps.data_ptr(), lengths.data_ptr(), scores.data_ptr(), cursors.data_ptr(),
                                                          ptr(fr), ptr(du), *self._tail()), "compute_rnnt_tdt_beam_results")
        torch.cuda.synchronize()
        return tuple(None if x is None else x.cpu().numpy() for x in (hyps, lengths, scores, cursors, fr, du))


class PyBeam:
    """The same caller through tdt.TDTBeamJoint (the engine route)."""

    def __init__(self, sc):
        self.case = sc.case
        self.jb = tdt.TDTBeamJoint(DeviceJoint(sc.case), sc.case.durations, sc.K, joint_dtype=("f32", "f16")[sc.case.dtype], token_times=True)
        assert self.jb.engine and self.jb.Jp == sc.case.J

    def begin(self):
        self.jb.begin(_dev(self.case.enc_proj), torch.tensor(self.case.frames))

    def step(self, rows):
        parents, emitted = self.jb.step(pred_proj=_dev(rows))
        return parents.cpu().numpy(), emitted.cpu().numpy()

    def results(self):
        out = self.jb.results()
        cpu = lambda x: x.cpu().numpy()  # noqa: E731
        return tuple(cpu(x) for x in out[:3]) + (cpu(self.jb.cursors()),) + tuple(cpu(x) for x in out[3:])


def _checked(sc, engine=None, fn=None, **kw):
    fn = fn or LogitsEntry(sc.case)
    trace, ref, worst, bar = bc.run_tdt_beam(engine or AbiBeam(sc), sc, fn, **kw)
    print(bc.describe(sc, ref.ev, worst, bar), f"logits-calls={fn.calls}")
    return trace, ref, fn


def random_model(name, dtype, J, V, durations, K, B, T, frames, blank, seeds, steps=None, big=()):
    """The first seed of `seeds` whose random model keeps the restatement's gap precondition on the logits entry's own logits."""
    for seed in seeds:
        case = random_case(f"{name}-seed{seed}", dtype, J, V, durations, B, T, frames, blank, seed, big=big)
        sc = bc.Scenario(case.name, case, K, T if steps is None else steps)
        fn = LogitsEntry(case)
        try:
            bc.dry_run(sc, fn)
        except AssertionError as e:
            if "scenario precondition" not in str(e):
                raise
            continue
        return sc, fn
    raise AssertionError(f"{name}: no seed of {list(seeds)} keeps the gap precondition")


# ---- the step's diagnostics ---------------------------------------------------------------------------
def _diagnostics(case, K, T, bitwise=True):
    """Follow the engine's own decisions for T steps; at every step every ACTIVE row's listed token logits, duration logits and
    logsumexps against the logits entry for that hypothesis alone.  -> active rows checked."""
    sc = bc.Scenario(case.name, case, K, T)
    fn = LogitsEntry(case)
    eng = AbiBeam(sc, diag=True, poison=True)
    eng.begin()
    B, V = case.B, case.V
    seqs = [()] * (B * K)
    Tb = [min(max(int(f), 0), case.maxT) for f in case.frames]
    checked = 0
    for t in range(T):
        _, _, scores, cursors, _, _ = eng.results()
        active = [b * K + k for b in range(B) for k in range(K) if t < Tb[b] and scores[b, k] > -math.inf and cursors[b, k] == t]
        rows = np.full((B * K, case.J), np.nan, np.float32)
        for r in active:
            rows[r] = case.pred_row(r // K, t, seqs[r])
        for x in eng.diag:
            x.fill_(float("nan") if x.dtype == torch.float32 else -7)
        parents, emitted = eng.step(rows)
        tl, ts, dl, lse = (x.cpu().numpy() for x in eng.diag)
        for r in range(B * K):
            if r not in active:  # written for the rows that were active alone
                assert np.isnan(tl[r]).all() and (ts[r] == -7).all() and np.isnan(dl[r]).all() and np.isnan(lse[r]).all(), (t, r)
                continue
            lg = fn(r // K, t, seqs[r])
            tok, dur = lg[:V], lg[V:]
            order = sorted(range(V), key=lambda v: (-float(tok[v]), v))[:K]
            n = min(K, V)
            assert ts[r, :n].tolist() == order and (ts[r, n:] == -1).all() and np.isneginf(tl[r, n:]).all(), (t, r, ts[r], order)
            if bitwise:
                assert tl[r, :n].tobytes() == tok[order].tobytes(), (t, r, "token logits")
                assert dl[r].tobytes() == dur.tobytes(), (t, r, "duration logits")
            else:  # DT 2 (J = 704): the shared joint sits ~1e-7 off the logits entry on a few symbols (tests/test_beam_search_gpu.py)
                assert (np.abs(tl[r, :n] - tok[order]) <= 1e-6 * np.maximum(1.0, np.abs(tok[order]))).all(), (t, r)
                assert (np.abs(dl[r] - dur) <= 1e-6 * np.maximum(1.0, np.abs(dur))).all(), (t, r)
            for got, head in ((lse[r, 0], tok), (lse[r, 1], dur)):
                want = tc._logsumexp(head.astype(np.float64))
                assert abs(float(got) - want) <= 1e-6 * max(1.0, abs(want)), (t, r, float(got), want)
            checked += 1
        seqs = [seqs[p] + ((e,) if e >= 0 else ()) for p, e in zip(parents.tolist(), emitted.tolist())]
    return checked


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("split", list(SPLITS), ids=[f"V{v}-D{d}" for v, d in SPLITS])
def test_step_diagnostics_are_the_logits_entry_s_bitwise(split, where):
    V, D = split
    dtype, J = SPLITS[split]
    blank = {"first": 0, "middle": V // 2, "last": V - 1}[where]
    dur = {1: D1, 5: D5, 8: D8}[D]
    T = 9 if J < 640 else 5
    case = random_case(f"diag-V{V}-D{D}-blank{blank}", dtype, J, V, dur, 3, T, [T, 4, T + 2], blank, 100 * V + D)
    checked = _diagnostics(case, 4, T)
    print(f"[{case.name}] active rows checked: {checked}")
    assert checked >= 8


def test_step_diagnostics_dt2_at_joint_size_704():
    case = random_case("diag-dt2-J704", 0, 704, 27, D5, 3, 6, [6, 3, 8], 13, 7)
    assert _diagnostics(case, 4, 6, bitwise=False) >= 6


# ---- row tiles ----------------------------------------------------------------------------------------
def test_a_full_row_tile_and_one_row_with_both_tanh_routes():
    """B beam = 33 rows: a full tile and one row of a second; utterance 1's enc_proj and utterance 2's pred_proj leave the e^{2x}
    table range (the direct-tanh route beside the table route in one tile)."""
    frames = [(5, 2, 7, 0, 3)[b % 5] for b in range(33)]
    sc, fn = random_model("tiles-33x1", 1, 128, 126, D5, 1, 33, 5, frames, 0, range(33, 43), big=(1, 2))
    _, ref, _ = _checked(sc, fn=fn)
    assert ref.ev.active_rows >= 33
    assert _diagnostics(random_case("tiles-33x1-diag", 0, 64, 27, D5, 33, 4, [4] * 33, 26, 34, big=(1, 2)), 1, 4) >= 33
    # 11 utterances x beam 3 = 33 rows: the second tile holds the last hypothesis of the last beam
    sc, fn = random_model("tiles-11x3", 0, 64, 27, D5, 3, 11, 5, [(5, 3, 0, 6)[b % 4] for b in range(11)], 3, range(50, 60), big=(1, 2))
    _checked(sc, fn=fn)


def test_beam_16_with_a_tile_of_waiting_and_a_tile_of_frozen_rows():
    """long-jumps at beam 16, 4 utterances = 64 rows: tile 0 (utterances 0, 1) waits through the idle frames between two jumps with
    both beams full, tile 1 (T_b = 0 and T_b = 1) is frozen from frame 1 on.  NaN pred_proj rows prove that they read nothing."""
    for dtype in (0, 1):
        sc = bc.long_jump_scenario(16, dtype)
        _, ref, _ = _checked(sc)
        bc.check_expectations(sc, ref.ev)
        assert ref.ev.idle_full >= 4
    sc, fn = random_model("beam16", 1, 128, 1030, D5, 16, 3, 6, [6, 0, 4], 515, range(7, 17))
    _, ref, _ = _checked(sc, fn=fn)
    assert ref.ev.full_frames >= 4


# ---- the scripted scenarios ----------------------------------------------------------------------------
SCRIPTED = bc.scripted_scenarios(0) + bc.scripted_scenarios(1)


@pytest.mark.parametrize("route", ["abi", "python"])
@pytest.mark.parametrize("sc", SCRIPTED, ids=[s.name for s in SCRIPTED])
def test_scripted_scenarios(sc, route):
    _, ref, _ = _checked(sc, AbiBeam(sc) if route == "abi" else PyBeam(sc))
    bc.check_expectations(sc, ref.ev)


def test_hash_collision_does_not_merge():
    sc, want0, want1 = bc.collision_scenario()
    trace, ref, _ = _checked(sc, every_step=False)
    hyps, lengths = trace[-1][0], trace[-1][1]
    assert lengths[0].tolist() == [1280, 1280] and ref.ev.merges == 0
    assert hyps[0, 0, :1280].tolist() == list(want0) and hyps[0, 1, :1280].tolist() == list(want1)


# ---- random models ----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("shape", [(27, 5, 64, 0), (126, 5, 128, 1), (1030, 5, 128, 1)], ids=str)
def test_random_models_against_the_restatement(shape, K):
    V, D, J, dtype = shape
    sc, fn = random_model(f"random-V{V}-J{J}-K{K}", dtype, J, V, D5, K, 3, 9, [9, 0, 6], V // 3, range(1000 + V + K, 1000 + V + K + 20))
    _, ref, _ = _checked(sc, fn=fn)
    assert ref.ev.active_rows >= 2 * K and ref.ev.merges + ref.ev.kept_apart >= 1


def test_beam_1_equals_tdt_greedy_on_the_engine():
    """ids and frames bitwise, scores within the bar: the argmaxes of the two heads are the argmax of the sum."""
    for dtype, J, V in ((0, 64, 27), (1, 128, 126)):
        case = random_case(f"beam1-dt{dtype}", dtype, J, V, D5, 5, 9, [9, 4, 0, 12, 1], 2, 4242 + dtype)
        joint = DeviceJoint(case)
        B, T = case.B, case.maxT
        enc, frames = _dev(case.enc_proj), torch.tensor(case.frames)
        jd = ("f32", "f16")[dtype]
        jb = tdt.TDTBeamJoint(joint, D5, 1, joint_dtype=jd, token_times=True)
        jg = tdt.TDTGreedyJoint(joint, D5, joint_dtype=jd, token_times=True)
        jb.begin(enc, frames)
        jg.begin(enc, frames, None, 1, T)
        stats = torch.zeros(B, 4, device=DEV)
        yb, yg, max_lse, steps = [()] * B, [()] * B, 0.0, [0] * B
        # (random_case's pred_proj rows depend on the tokens alone, not on the frame)
        rows = lambda ys: _dev(np.stack([case.pred_row(b, 0, ys[b]) for b in range(B)]))  # noqa: E731
        for t in range(T):
            _, em = jb.step(pred_proj=rows(yb))
            yb = [y + ((int(e),) if e >= 0 else ()) for y, e in zip(yb, em.tolist())]
        while int(jg.all_done.cpu()[0]) == 0:
            stats.fill_(float("nan"))  # (written for the hypotheses that ran)
            em = jg.step(pred_proj=rows(yg), logit_stats=stats)
            st = stats.cpu().numpy()
            for b in range(B):
                if st[b, 1] == st[b, 1]:
                    steps[b] += 1
                    max_lse = max(max_lse, abs(float(st[b, 1])), abs(float(st[b, 3])))
            yg = [y + ((int(e),) if e >= 0 else ()) for y, e in zip(yg, em.tolist())]
        hyps, lengths, scores, fr, du = (x.cpu() for x in jb.results())
        gl, gh, gf, gs = jg.lengths.cpu(), jg.hyps.cpu(), jg.frames.cpu(), jg.scores.cpu()
        assert lengths[:, 0].tolist() == gl.tolist() and int(gl.sum()) >= 5
        for b in range(B):
            n = int(gl[b])
            assert hyps[b, 0, :n].tolist() == gh[b, :n].tolist() and fr[b, 0, :n].tolist() == gf[b, :n].tolist(), (dtype, b)
            # (each decoder is within the bar of the exact score, so the two are within twice the bar of each other)
            err, bar = abs(float(scores[b, 0]) - float(gs[b])), 2 * bc.score_bar(max(steps[b], 1), max_lse, float(gs[b]))
            assert err <= bar, (dtype, b, float(scores[b, 0]), float(gs[b]), err, bar)


# ---- robustness --------------------------------------------------------------------------------------
def test_determinism_side_stream_poisoned_and_reused_workspaces():
    sc = bc.random_scenario([0, 1, 2, 3, 4], 4, 1)
    fn = LogitsEntry(sc.case)
    first, _, _ = _checked(sc, fn=fn)
    again = bc.run_tdt_beam(AbiBeam(sc), sc, fn, check=False)[0]
    assert bc.traces_equal(first, again), "two decodes of the same input differ"
    poisoned = bc.run_tdt_beam(AbiBeam(sc, poison=True), sc, fn, check=False)[0]
    assert bc.traces_equal(first, poisoned), "a workspace of 0xFF bytes changed the decode"
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = bc.run_tdt_beam(AbiBeam(sc, stream=side), sc, fn, check=False)[0]
    assert bc.traces_equal(first, other), "a side stream changed the decode"
    # a workspace left behind by a larger decode of another shape
    big = bc.random_scenario([0, 1, 2], 16, 1)
    eng = AbiBeam(big)
    assert eng.ws.numel() > _lib.tdt_beam_workspace_bytes(sc.case.maxT, sc.case.B, sc.K, sc.case.J, sc.case.V, sc.case.D, 1, True)
    bc.run_tdt_beam(eng, big, LogitsEntry(big.case), check=False)
    reused = bc.run_tdt_beam(AbiBeam(sc, ws=eng.ws), sc, fn, check=False)[0]
    assert bc.traces_equal(first, reused), "a reused workspace changed the decode"
    # untimed: the same decisions and scores
    plain = bc.run_tdt_beam(AbiBeam(sc, timed=False), sc, fn, check=False)[0]
    for a, b in zip(first, plain):
        for x, y in zip(a[:4], b[:4]):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_an_utterance_alone_equals_the_same_one_in_the_batch():
    sc = bc.random_scenario([0, 1, 2, 3, 4], 4, 0)
    case = sc.case
    full = bc.run_tdt_beam(AbiBeam(sc), sc, LogitsEntry(case), check=False)[0][-1]
    for b in (0, 3, 4):
        one = tc.scripted_case("alone", 0, case.V, case.durations, 1, case.maxT, [case.frames[b]], None, 1, case.blank,
                               lambda _b, t, y, b=b: case.script(b, t, y), [case.maxT])
        s1 = bc.Scenario("alone", one, sc.K, sc.steps)
        alone = bc.run_tdt_beam(AbiBeam(s1), s1, LogitsEntry(one), check=False)[0][-1]
        for x, y in zip(alone, full):
            assert x[0].tobytes() == y[b].tobytes(), b  # ids, lengths, scores (as bits), cursors, frames, durations


def test_python_workspace_fill_and_reuse(monkeypatch):
    pred, joint = _device_model()
    enc, frames = _enc(5, 12)
    tdt._BEAM_WORKSPACES.clear()
    fresh = tdt.tdt_beam_search_batch(pred, joint, enc, frames, D5, beam=4, token_times=True)
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", 0xFF)
    poisoned = tdt.tdt_beam_search_batch(pred, joint, enc, frames, D5, beam=4, token_times=True)
    monkeypatch.setattr(jmod, "_WORKSPACE_FILL", None)
    for a, b in zip(fresh, poisoned):
        assert torch.equal(a, b)


# ---- tdt_beam_search_batch -----------------------------------------------------------------------------
def _device_model():
    pred, joint = small_tdt_model(3)
    return pred.to(DEV), joint.to(DEV)


def _enc(B, T):
    enc = torch.randn(B, T, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    return enc, torch.tensor([12, 7, 0, 1, 9][:B], dtype=torch.int32, device=DEV)


def test_no_host_sync_per_step():
    pred, joint = _device_model()
    enc, frames = _enc(5, 12)
    for route in ("torch", "engine"):
        tdt.tdt_beam_search_batch(pred, joint, enc, frames, D5, beam=4, prediction_route=route)  # (allocations)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = tdt.tdt_beam_search_batch(pred, joint, enc, frames, D5, beam=4, prediction_route=route)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        ref = tdt.tdt_beam_search_batch(pred, joint, enc, frames, D5, beam=4, prediction_route=route)
        for a, b in zip(out, ref):
            assert torch.equal(a, b)


@pytest.mark.parametrize("route", ["torch", "engine"])
def test_search_batch_on_both_prediction_routes(route):
    """Sorted n-best lists whose frames respect the jumps; beam = 1 equal to tdt_greedy_search_batch(max_symbols_per_frame=1) in
    ids and frames; fewer joint rows than occupied slots; the engine ran (no torch fall-back on the device)."""
    pred, joint = _device_model()
    enc, frames = _enc(5, 12)
    assert tdt.TDTBeamJoint(joint, D5, 4).engine
    hyps, lengths, scores, fr, du = tdt.tdt_beam_search_batch(pred, joint, enc, frames, D5, beam=4, prediction_route=route,
                                                              token_times=True, count_active=True)
    active = tdt.LAST_ACTIVE_ROWS.cpu()
    hyps, lengths, scores, fr, du = (x.cpu() for x in (hyps, lengths, scores, fr, du))
    assert (active <= 4 * frames.cpu()).all() and int(active[0]) >= 1 and int(active[2]) == 0
    assert lengths[2].tolist() == [0, 0, 0, 0] and scores[2, 0] == 0 and (scores[2, 1:] == -math.inf).all()
    for b in range(5):
        s = scores[b].tolist()
        assert s == sorted(s, reverse=True)
        for k in range(4):
            n = int(lengths[b, k])
            assert (fr[b, k, :n] < frames[b].item()).all() and (du[b, k, :n] >= 1).all()
            assert n < 2 or (fr[b, k, 1:n] >= fr[b, k, : n - 1] + du[b, k, : n - 1]).all()
            assert (fr[b, k, n:] == -1).all() and (du[b, k, n:] == -1).all() and not hyps[b, k, n:].any()
    h1, l1, s1, f1, _ = (x.cpu() for x in tdt.tdt_beam_search_batch(pred, joint, enc, frames, D5, beam=1, prediction_route=route,
                                                                   token_times=True))
    hg, lg, sg, fg, _ = (x.cpu() for x in tdt.tdt_greedy_search_batch(pred, joint, enc, frames, D5, max_symbols_per_frame=1,
                                                                     prediction_route=route, token_times=True))
    assert l1[:, 0].tolist() == lg.tolist() and int(lg.sum()) >= 5
    for b in range(5):
        n = int(lg[b])
        assert h1[b, 0, :n].tolist() == hg[b, :n].tolist() and f1[b, 0, :n].tolist() == fg[b, :n].tolist()
    assert torch.allclose(s1[:, 0], sg, atol=1e-4)
    assert (scores[:, 0] >= s1[:, 0] - 1e-4).all()
