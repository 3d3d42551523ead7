"""Streaming beam search (decoding.StreamingBeamDecoder, include/rnnt.h compute_rnnt_beam_stream_*), CPU side: the torch route's
state machine in float64 -- chunking equivalence in slot k of 16 under other traffic, the offline decoder and an independent
restatement, beam = 1 against the streaming greedy decoder, the capacity rule, stable_lengths, finished and reset slots, the
argument checks of feed -- and the C ABI's argument checks of the new entry points (no device needed)."""
import ctypes
import math
import random

import pytest
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib, decoding
from rnnt_speech_recognition_amd.decoding import StreamingBeamDecoder, StreamingGreedyDecoder
from tests.test_beam_search import restate
from tests.test_frontend import small_model
from tests.test_streaming_greedy import chunkings

LENGTHS = [30, 25, 17, 9, 22, 30, 13, 27]
SLOTS = [15, 3, 7, 0, 9, 12, 1, 4]


def beam_model(seed=5, dtype=torch.float64, device="cpu"):
    model = small_model(seed)
    with torch.no_grad():
        model.joint.b2[0] += 0.5  # blank-leaning: blank and symbol extensions in every beam, so merges happen
    return model.to(device=device, dtype=dtype).eval()


def common_prefix(rows):
    """rows: token lists of the occupied hypotheses -> length of their longest common prefix (0 for none)."""
    if not rows:
        return 0
    n = 0
    while all(n < len(r) for r in rows) and all(r[n] == rows[0][n] for r in rows):
        n += 1
    return n


def read_nbest(dec, slot):
    """-> (token lists of the occupied hypotheses, lengths [K], scores [K] (cloned), stable) of one slot; 5(b) on the way."""
    ids, lengths, scores = dec.nbest()
    stable = int(dec.bj.results()[3][slot])
    rows = [ids[slot, k, : int(lengths[slot, k])].tolist() for k in range(dec.K) if math.isfinite(float(scores[slot, k]))]
    assert stable == common_prefix(rows), (slot, stable, rows)
    assert stable <= min([len(r) for r in rows], default=0)
    for k in range(dec.K):
        assert not ids[slot, k, int(lengths[slot, k]):].any(), "zero padding"
    return rows, lengths[slot].clone(), scores[slot].clone(), stable


def one_call(model, x, K, N):
    dec = StreamingBeamDecoder(model, 1, x.shape[0], beam=K, max_length=N)
    dec.start([0])
    best, n, stable = dec.feed(x[None], [x.shape[0]], [True])
    out = read_nbest(dec, 0)
    assert best[0, : int(n[0])].tolist() == (out[0][0] if out[0] else []) and int(stable[0]) == out[3]
    return out


def run_schedule(model, streams, S, Tc, K, N, plans, seed=0, extra_restart=None):
    """tests/test_streaming_greedy.py run_schedule for the beam decoder.  plans[i] = (slot, start_feed, chunk lengths).  -> per
    stream its n-best (read_nbest) right after its final feed; stable_lengths is checked after every feed of every live slot."""
    rng = random.Random(seed)
    dec = StreamingBeamDecoder(model, S, Tc, beam=K, max_length=N)
    F = streams[0].shape[1]
    state = [dict(pos=0, k=0, started=False, done=False) for _ in streams]
    results, feed_no = {}, 0
    while not all(s["done"] for s in state):
        to_start = [i for i, (slot, sf, _) in enumerate(plans) if sf == feed_no]
        if to_start:
            dec.start([plans[i][0] for i in to_start])
            for i in to_start:
                state[i]["started"] = True
        if extra_restart is not None and extra_restart[0] == feed_no:
            dec.start([extra_restart[1]])
        mel = torch.randn(S, Tc, F, dtype=streams[0].dtype, device=streams[0].device)  # (garbage past each slot's frames)
        frames, final, owner = [0] * S, [False] * S, {}
        for i, (slot, _, chunks) in enumerate(plans):
            st = state[i]
            if not st["started"] or st["done"] or (feed_no % 3 == 1 and rng.random() < 0.5):
                continue  # not yet started, finished, or sitting this feed out (an idle feed: 0 frames)
            c = chunks[st["k"]]
            mel[slot, :c] = streams[i][st["pos"]: st["pos"] + c]
            frames[slot], final[slot] = c, st["k"] == len(chunks) - 1
            owner[slot] = i
            st["pos"] += c
            st["k"] += 1
        best, n, stable = dec.feed(mel, frames, final)
        for slot, i in owner.items():
            out = read_nbest(dec, slot)
            assert best[slot, : int(n[slot])].tolist() == (out[0][0] if out[0] else []) and int(stable[slot]) == out[3]
            if final[slot]:
                state[i]["done"] = True
                results[i] = out
        feed_no += 1
    return results


def plans_for(lengths, f, kind, seed, slots):
    rng = random.Random(seed)
    plans = [(slots[i], i % 4, chunkings(L, f, rng)[kind]) for i, L in enumerate(lengths)]
    return plans, max(max(p[2]) for p in plans)


def has_odd_chunk(plans, f):
    """the parity hazard: a non-final chunk with an odd number of ENCODER frames (the double-buffer side must not follow it)"""
    return any((-(-c // f)) % 2 == 1 for _, _, chunks in plans for c in chunks[:-1])


def _streams(model, lengths, seed, device="cpu"):
    torch.manual_seed(seed)
    p = next(model.parameters())
    return [torch.randn(L, model.encoder.input_norm.num_features, dtype=p.dtype).to(device) for L in lengths]


def seeded_streams(model, lengths, seeds, device="cpu"):
    """one seed per stream, so that a stream with a near-tie can be replaced without moving the others"""
    return [_streams(model, [L], seed, device)[0] for L, seed in zip(lengths, seeds)]


# ---- check 2: chunking equivalence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4, 8])
def test_chunked_streams_in_slot_k_of_16_equal_one_call(K):
    model = beam_model()
    f = model.encoder.reduce.factor
    X = _streams(model, LENGTHS, 21)
    N = 24
    want = [one_call(model, x, K, N) for x in X]
    assert sum(len(w[0][0]) for w in want) >= 10
    odd = False
    for kind in ["one", "f", "random"]:
        plans, Tc = plans_for(LENGTHS, f, kind, 5, SLOTS)
        odd |= has_odd_chunk(plans, f)
        got = run_schedule(model, X, 16, Tc, K, N, plans, seed=len(kind), extra_restart=(2, 11))  # slot 11: restarted, never fed
        for i in range(len(X)):
            rows, lengths, scores, stable = got[i]
            assert rows == want[i][0] and torch.equal(lengths, want[i][1]) and stable == want[i][3], (kind, i)
            fin = torch.isfinite(want[i][2])
            assert torch.equal(torch.isfinite(scores), fin)
            assert (scores[fin] - want[i][2][fin]).abs().max() <= 1e-12, (kind, i)  # (the engine: bitwise)
    assert odd, "no chunk with an odd number of encoder frames: the schedule does not exercise the buffer-side parity"


# ---- check 3: the offline decoder, an independent restatement, beam = 1 against greedy ----------------------------------------
SEEDS = {1: 5, 4: 5, 8: 5}  # model seed per K, chosen on this mirror: the deciding gaps clear twice the bar


@pytest.mark.parametrize("K", [1, 4, 8])
def test_streams_match_the_offline_decoder_and_a_restatement(K):
    model = beam_model(SEEDS[K])
    f = model.encoder.reduce.factor
    lengths = LENGTHS[:5]
    X = _streams(model, lengths, 21)
    plans, Tc = plans_for(lengths, f, "random", 5, SLOTS)
    got = run_schedule(model, X, 16, Tc, K, 24, plans, seed=3)
    bar = 1e-9
    for i, x in enumerate(X):
        with torch.no_grad():
            enc = model.encoder(x[None])
        ids, n, sc = decoding.beam_search_batch(model, enc, torch.tensor([enc.shape[1]]), beam=K)
        rows, lengths_k, scores, _ = got[i]
        assert rows[0] == ids[0, 0, : int(n[0, 0])].tolist(), i
        want, _, gap = restate(model, enc[0], K, 0)
        assert gap > 2 * bar, f"stream {i}: deciding candidates {gap:.3e} apart: pick another seed"
        assert len(rows) == len(want)
        for k, (y, s) in enumerate(want):
            assert rows[k] == list(y), (i, k)
            assert abs(float(scores[k]) - s) <= bar * max(1.0, abs(s)), (i, k)


def test_beam_one_is_streaming_greedy_with_one_symbol_per_frame():
    model = beam_model()
    f = model.encoder.reduce.factor
    X = _streams(model, LENGTHS[:4], 8)
    plans, Tc = plans_for(LENGTHS[:4], f, "random", 2, [2, 0, 3, 1])
    got = run_schedule(model, X, 4, Tc, 1, 24, plans)
    for i, x in enumerate(X):
        g = StreamingGreedyDecoder(model, 1, x.shape[0], max_length=None, max_symbols_per_frame=1)
        g.start([0])
        g.feed(x[None], [x.shape[0]], [True])
        ids, n, _ = g.hypotheses()
        assert got[i][0][0] == ids[0, : int(n[0])].tolist() and int(got[i][1][0]) == int(n[0]), i


# ---- check 5: the new rules -----------------------------------------------------------------------------------------------
def restate_capped(model, enc_b, K, blank, cap):
    """tests/test_beam_search.py restate with the stream's capacity rule: a hypothesis of cap tokens offers blank alone."""
    beam = [((), 0.0)]
    for i in range(enc_b.shape[0]):
        cands = []
        for hi, (y, s) in enumerate(beam):
            g = model.prediction(torch.tensor([(0,) + y]))[:, -1:, :]
            logits = model.joint.logits(enc_b[None, i: i + 1], g)[0, 0, 0].double()
            lse = float(torch.logsumexp(logits, 0))
            for v in ([blank] if len(y) >= cap else range(logits.shape[0])):
                cands.append((s + (float(logits[v]) - lse), hi, v))
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        merged, order = {}, []
        for sc, hi, v in cands[:K]:
            y = beam[hi][0] if v == blank else beam[hi][0] + (v,)
            if y in merged:
                a = merged[y]
                merged[y] = max(a, sc) + math.log1p(math.exp(min(a, sc) - max(a, sc)))
            else:
                merged[y] = sc
                order.append(y)
        beam = sorted(((y, merged[y]) for y in order), key=lambda e: -e[1])
    return beam


@pytest.mark.parametrize("K", [1, 4])
def test_capacity_rule_stops_hypotheses_at_max_length(K):
    model = beam_model()
    with torch.no_grad():
        model.joint.b2[0] -= 6.0  # every frame prefers a symbol: without the rule a hypothesis would grow every frame
    f = model.encoder.reduce.factor
    x = _streams(model, [30], 4)[0]
    N = 5
    dec = StreamingBeamDecoder(model, 2, 8, beam=K, max_length=N)
    dec.start([1])
    seen = []
    for k, c in enumerate([8, 8, 8, 6]):
        mel = torch.zeros(2, 8, x.shape[1], dtype=x.dtype)
        mel[1, :c] = x[8 * k: 8 * k + c]
        dec.feed(mel, [0, c], [False, k == 3])
        seen.append(read_nbest(dec, 1))
    rows, lengths, scores, _ = seen[-1]
    assert all(len(r) == N for r in rows) and int(lengths.max()) == N
    assert seen[1][0][0] == seen[-1][0][0] and float(seen[-1][2][0]) < float(seen[1][2][0])  # full after 8 frames; blanks go on
    with torch.no_grad():
        enc = model.encoder(x[None])[0]
    want = restate_capped(model, enc, K, 0, N)
    assert [list(y) for y, _ in want] == rows
    for k, (_, s) in enumerate(want):
        assert abs(float(scores[k]) - s) <= 1e-9 * max(1.0, abs(s))
    ids = dec.nbest()[0]
    assert ids.shape == (2, K, N)


def check_finished_and_reset_slots(model, device="cpu"):
    """5(c): a reset slot beside live slots leaves them bitwise unchanged; a finished slot ignores feeds until start."""
    X = _streams(model, [16, 16], 6, device)
    F = X[0].shape[1]

    def run(disturb):
        dec = StreamingBeamDecoder(model, 3, 8, beam=4, max_length=16)
        dec.start([0, 2])
        outs = []
        for k in range(2):
            mel = torch.zeros(3, 8, F, dtype=X[0].dtype, device=device)
            mel[0], mel[2] = X[0][8 * k: 8 * k + 8], X[1][8 * k: 8 * k + 8]
            if disturb and k == 1:
                dec.start([1])  # a reset slot beside live slots
                mel[1] = 1.0
            dec.feed(mel, [8, 8 if disturb and k == 1 else 0, 8], [k == 1, False, k == 1])
            outs.append([read_nbest(dec, s) for s in (0, 2)])
        return dec, outs

    dec, plain = run(False)
    _, disturbed = run(True)
    for a, b in zip(plain, disturbed):
        for (r0, l0, s0, st0), (r1, l1, s1, st1) in zip(a, b):
            assert r0 == r1 and torch.equal(l0, l1) and torch.equal(s0, s1) and st0 == st1
    # a never-started slot: empty; finished slots: frozen by further feeds, until start
    rows, lengths, scores, stable = read_nbest(dec, 1)
    assert rows == [] and not lengths.any() and bool(torch.isinf(scores).all()) and stable == 0
    before = [read_nbest(dec, s) for s in (0, 2)]
    mel = torch.randn(3, 8, F, dtype=X[0].dtype).to(device)
    dec.feed(mel, [8, 0, 8], [False, False, True])
    after = [read_nbest(dec, s) for s in (0, 2)]
    for (r0, l0, s0, st0), (r1, l1, s1, st1) in zip(before, after):
        assert r0 == r1 and torch.equal(l0, l1) and torch.equal(s0, s1) and st0 == st1
    dec.start([0])
    rows, lengths, scores, stable = read_nbest(dec, 0)
    assert rows == [[]] and float(scores[0]) == 0.0 and stable == 0
    assert read_nbest(dec, 2)[0] == before[1][0]


def test_finished_slots_ignore_feeds_and_resets_leave_neighbours_alone():
    check_finished_and_reset_slots(beam_model())


def test_feed_checks_its_arguments():
    model = beam_model()
    f = model.encoder.reduce.factor
    F = model.encoder.input_norm.num_features
    with pytest.raises(ValueError):
        StreamingBeamDecoder(model, 65, 8, beam=16)  # slots * beam > 1024
    with pytest.raises(ValueError):
        StreamingBeamDecoder(model, 2, 8, beam=17)
    with pytest.raises(ValueError):
        StreamingBeamDecoder(model, 2, 8, beam=4, max_length=0)
    dec = StreamingBeamDecoder(model, 2, 8, beam=2)
    assert dec.max_length == StreamingBeamDecoder.DEFAULT_MAX_LENGTH and pkg.StreamingBeamDecoder is StreamingBeamDecoder
    x = torch.zeros(2, 8, F, dtype=torch.float64)
    with pytest.raises(ValueError):
        dec.feed(torch.zeros(2, 9, F, dtype=torch.float64), [8, 8], [False, False])  # more than max_chunk_frames
    with pytest.raises(ValueError):
        dec.feed(x, [f + 1, 0], [False, False])  # a non-final chunk that is no multiple of the reduction factor
    with pytest.raises(ValueError):
        dec.feed(x, [8], [False])
    with pytest.raises(ValueError):
        dec.start([2])


# ---- check 6: the boundary of the C ABI ---------------------------------------------------------------------------------------
def test_argument_validation_needs_no_device():
    pkg.build()
    lib = _lib.load()
    fake, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)  # never dereferenced: every call below is rejected before any launch
    o = _lib.make_options(0, 0, 8, 1)
    n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
    size = lib.get_rnnt_beam_stream_workspace_size
    assert size(8, 16, 4, 100, 640, 640, 4096, 1, ctypes.byref(n)) == 0 and n.value > 0 and n.value % 256 == 0
    assert size(8, 16, 4, 400, 640, 640, 4096, 1, ctypes.byref(m)) == 0 and m.value % 256 == 0
    assert m.value - n.value >= 2 * 16 * 4 * 300 * 4  # grows with N: 2 S K N token words
    assert size(8, 16, 8, 100, 640, 640, 4096, 1, ctypes.byref(m)) == 0 and m.value > n.value and m.value % 256 == 0  # and with K
    assert size(8, 64, 16, 100, 640, 640, 4096, 1, ctypes.byref(m)) == 0  # S K = 1024
    assert size(8, 16, 4, 100, 640, 640, 4096, 1, None) == 2
    for args in ((8, 16, 0, 100, 640, 640, 28, 0), (8, 16, 17, 100, 640, 640, 28, 0), (8, 65, 16, 100, 640, 640, 28, 0),
                 (8, 0, 4, 100, 640, 640, 28, 0), (8, 16, 4, 0, 640, 640, 28, 0), (0, 16, 4, 100, 640, 640, 28, 0),
                 (8, 16, 4, 100, 0, 640, 28, 0), (8, 16, 4, 100, 4097, 640, 28, 0), (8, 16, 4, 100, 640, 96, 28, 0),
                 (8, 16, 4, 100, 640, 640, 28, 0x100), (8, 16, 4, 100, 640, 640, 28, 2), (8, 64, 16, 1 << 21, 640, 640, 28, 0)):
        assert size(*args, ctypes.byref(m)) == 2, args

    def begin(w1=fake, b1=fake, w2=fake, b2=fake, H=640, J=640, V=28, S=16, K=4, N=100, dt=0, ws=fake, opts=o):
        return lib.compute_rnnt_beam_stream_begin(w1, b1, w2, b2, H, J, V, S, K, N, dt, ws, opts)

    def feed(enc=fake, Te=8, cf=fake, rs=None, fi=None, H=640, J=640, V=28, S=16, K=4, N=100, dt=0, ws=fake, opts=o):
        return lib.compute_rnnt_beam_stream_feed(enc, Te, cf, rs, fi, H, J, V, S, K, N, dt, ws, opts)

    def step(pp=fake, par=fake, em=fake, tl=None, ts=None, lse=None, J=640, V=28, S=16, K=4, N=100, dt=0, ws=fake, opts=o, **_):
        return lib.compute_rnnt_beam_stream_step(pp, par, em, tl, ts, lse, J, V, S, K, N, dt, ws, opts)

    def results(h=fake, hl=fake, sc=fake, stb=None, J=640, V=28, S=16, K=4, N=100, dt=0, ws=fake, opts=o, **_):
        return lib.compute_rnnt_beam_stream_results(h, hl, sc, stb, J, V, S, K, N, dt, ws, opts)

    cpu = _lib.make_options(0, 0, 8, 1, loc=_lib.RNNT_CPU)
    for call in (begin, feed, step, results):
        assert call(opts=cpu) == 2                       # device-only library
        assert call(opts=_lib.make_options(0, 28, 8, 1)) == 2  # blank_label >= alphabet_size
        assert call(opts=_lib.make_options(0, 0, 0, 1)) == 2   # max_chunk_frames = 0
        assert call(ws=None) == 2 and call(ws=ctypes.c_void_p(256 + 64)) == 2  # workspace NULL / not 256-byte aligned
        assert call(dt=0x100) == 2 and call(dt=3) == 2  # no flag bits
        assert call(K=0) == 2 and call(K=17) == 2
        assert call(S=65, K=16) == 2 and call(S=0) == 2  # S K > 1024
        assert call(N=0) == 2
        assert call(J=96) == 2 and call(V=4096) == 2
    assert begin(H=0) == 2 and begin(H=4097) == 2 and feed(H=0) == 2
    for k in ("w1", "b1", "w2", "b2"):
        assert begin(**{k: None}) == 2 and begin(**{k: odd}) == 2
    assert feed(Te=9) == 2 and feed(Te=-1) == 2 and feed(enc=None) == 2  # enc_frames > max_chunk_frames; frames without enc
    assert feed(cf=None) == 2
    for k in ("enc", "cf", "rs", "fi"):
        assert feed(**{k: odd}) == 2
    for k in ("pp", "par", "em"):
        assert step(**{k: None}) == 2
    for k in ("pp", "par", "em", "tl", "ts", "lse"):
        assert step(**{k: odd}) == 2
    for k in ("h", "hl", "sc"):
        assert results(**{k: None}) == 2
    for k in ("h", "hl", "sc", "stb"):
        assert results(**{k: odd}) == 2
