"""The streaming log-mel front end on the MI355X at the geometries the older suite never reaches (tests/frontend_geometry.py holds
the cases and the float64 restatement, tests/test_frontend_geometry.py proves on the CPU which geometry each case reaches):
every FFT size bin by bin, fe_frames_kernel<2048> included; mel widths on both sides of the 64-lane and 128-thread loop edges
and up to 1024; empty filters; stack and row_multiple up to 16 x 16 held frames; 0 ... 33 frames of different slots in one
launch; what only the C ABI can ask (clamped samples, NULL reset / final / audio, a reset of a live slot); step = 1, step = L =
nfft = 2048, one-sample chunks and 1024 slots.

Everything but the last group goes through the C ABI with geo.FrontEndCall: the workspace, rows_out and row_counts are 0xFF
bytes before begin (rows and counts again before every feed), the window, the mel matrix and the audio sit exactly to size in
front of NaN, and the audio is NaN beyond samples[s].

Bars: non-empty filters within frontend_cases.BAR (2e-3 on the log-mel value) of the float64 restatement; empty filters exactly
float32(log(1e-6)) with norm 0 and within the bar of the float64 running form with norm 1; counts equal to the integer mirror;
rows past a slot's count exact zeros out to max_rows and no poison left anywhere (FrontEndCall.feed asserts both on every
feed); what the header calls bitwise is compared with torch.equal.
The measured maxima are printed and, with FRONTEND_ACCURACY_DIR set, collected in frontend_geometry_accuracy.json in that
directory (kept in profiles/, with profiles/frontend_geometry_notes.md)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import frontend_cases as fc
from tests import frontend_geometry as geo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INVALID_VALUE = 2  # include/rnnt.h RNNT_STATUS_INVALID_VALUE


def _record(route, **figures):
    row = {k: float(v) for k, v in figures.items()}
    print(route, row)
    out = os.environ.get("FRONTEND_ACCURACY_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "frontend_geometry_accuracy.json")
    try:
        rows = json.load(open(path))
    except (OSError, ValueError):
        rows = {}
    rows[route] = row
    json.dump(rows, open(path, "w"), indent=1, sort_keys=True)


def _one_call(window, W, step, stack, rm, norm, audio):
    """The stream fed in one final call to a one-slot front end -> its rows [R, F]."""
    call = geo.FrontEndCall(window, W, len(audio), 1, step, stack, rm)
    rows, counts = call.feed([audio], [1], [1], norm)
    assert counts == [geo.frames_of(len(audio), len(window), step) // stack]
    return rows[0]


def _run_case(c, norm):
    """The case through the C ABI -> rows per stream slot; counts are compared with the mirror on every feed."""
    window, W = geo.tables(c)
    call = geo.FrontEndCall(window, W, c["K"], c["S"], c["step"], c["stack"], c["rm"])
    _, want = geo.mirror_of(c)
    got = {s: [] for s in c["streams"]}
    for i, (chunks, reset, final) in enumerate(geo.feeds_of(c)):
        rows, counts = call.feed(chunks, reset, final, norm)
        assert counts == want[i], (i, counts, want[i])
        for s in got:
            got[s].append(rows[s])
    return {s: torch.cat(v) for s, v in got.items()}


def _check_case(name, norm, bitwise=True):
    c = geo.CASES[name]
    window, W = geo.tables(c)
    rows = _run_case(c, norm)
    top = 0.0
    for s, r in rows.items():
        audio = geo.stream_audio(c, s)
        top = max(top, geo.check_rows(r.numpy(), audio, window, W, c["step"], c["stack"], norm))
        if bitwise and r.shape[0]:
            assert torch.equal(r, _one_call(window, W, c["step"], c["stack"], c["rm"], norm, audio)), (name, s)
    _record(f"{name} norm {norm}", max_err=top, bar=geo.BAR, rows=sum(r.shape[0] for r in rows.values()),
            empty_filters=len(geo.empty_filters(W)))
    return rows


# ---------------------------------------------------------------------------------------------
# 1. the spectrum, bin by bin
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L", sorted(geo.SPECTRUM))
def test_every_bin_of_the_spectrum(N, L):
    """W picks single bins, so rows are log(|X_k| + 1e-6) per bin: a wrong twiddle, bit-reversed index or a dropped Nyquist bin
    lands in its own column instead of being averaged over a band."""
    audio, window = geo.spectrum_audio(N, L), geo.spectrum_window(L)
    top, seen = 0.0, set()
    for M, off in geo.spectrum_pickers(N):
        W = geo.bin_picker(N // 2 + 1, M, off)
        call = geo.FrontEndCall(window, W, len(audio), 1, geo.SPECTRUM_STEP)
        rows, counts = call.feed([audio], [1], [1], norm=0)
        assert counts == [geo.SPECTRUM_FRAMES]
        want, _ = geo.log_mel64(audio, window, W, geo.SPECTRUM_STEP)
        err = np.abs(rows[0].numpy().astype(np.float64) - want)
        k = np.unravel_index(err.argmax(), err.shape)
        print(f"spectrum nfft {N} L {L} bins {off} ... {off + M - 1}: max error {err.max():.3e} at frame {k[0]} bin {k[1] + off}")
        assert err.max() < geo.BAR
        top = max(top, float(err.max()))
        seen |= set(range(off, off + M))
    assert seen == set(range(N // 2 + 1))
    _record(f"spectrum nfft {N} L {L}", max_err=top, bar=geo.BAR, bins=N // 2 + 1, frames=geo.SPECTRUM_FRAMES)


# ---------------------------------------------------------------------------------------------
# 2. mel widths, 3. stacking, 4. frame tiles within one call, 6. extremes: the case table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("name", sorted(k for k in geo.CASES if k.startswith("width_")))
def test_mel_widths(name, norm):
    _check_case(name, norm, bitwise=False)


@pytest.mark.parametrize("name", sorted(k for k in geo.CASES if k.startswith("stack")))
def test_stacking(name):
    """h0 climbs to G - 1 over feeds of 0, 1 or a few frames, feeds that emit nothing and several groups, a final partial group,
    and beside it a stream whose total stays below stack: bitwise the one-call rows, counts by the mirror on every feed."""
    rows = _check_case(name, 1)
    assert rows[0].shape[0] == 0 and rows[1].shape[0] > 0


def test_frame_tiles_of_different_slots_in_one_call():
    """Six slots complete 0, 1, 15, 16, 17 and 33 frames in one feed: the grid is sized by chunk_samples and whole workgroups
    return early for the shorter slots.  Each slot against the restatement and, bitwise, against the same slot fed alone."""
    rows = _check_case("tiles_0_1_15_16_17_33", 1)
    assert [rows[s].shape[0] for s in range(6)] == [0, 1, 15, 16, 17, 33]


def test_step_of_one_sample():
    """k samples give k frames; the float32 running mean over about 2,900 frames against the float64 one."""
    rows = _check_case("step1_L129", 1)
    assert rows[0].shape[0] == 2902


@pytest.mark.parametrize("norm", [0, 1])
def test_step_equal_to_length_equal_to_nfft_2048(norm):
    _check_case("step_eq_len_2048", norm)


def test_chunks_of_one_sample():
    """max_chunk_samples = 1: 140 feeds of one sample, the first frame with the 129th."""
    rows = _check_case("chunk1_L129", 1)
    assert rows[0].shape[0] == 3


def test_1024_slots():
    """Every 64th slot is live with its own stream; the others are finished and stay zero (FrontEndCall.feed asserts the zeros)."""
    rows = _check_case("slots1024", 1, bitwise=False)
    c = geo.CASES["slots1024"]
    window, W = geo.tables(c)
    for s in (0, 960):
        assert torch.equal(rows[s], _one_call(window, W, c["step"], 1, 1, 1, geo.stream_audio(c, s)))


# ---------------------------------------------------------------------------------------------
# 5. what only the C ABI can ask
# ---------------------------------------------------------------------------------------------
ABI = dict(sr=16000, L=400, step=160, M=20, stack=3, rm=2)


def _abi_tables():
    return geo.hann(ABI["L"]), geo.mel_weights(ABI["M"], 257, ABI["sr"], 125.0, 7600.0)


def test_samples_are_clamped_into_the_chunk():
    """samples[s] = -5 acts as 0 and samples[s] = chunk_samples + 100 as chunk_samples.  The audio is [S, chunk_samples] exactly,
    NaN behind it: for the last slot the clamp is what keeps the read inside the buffer."""
    window, W = _abi_tables()
    L, step, stack, rm = ABI["L"], ABI["step"], ABI["stack"], ABI["rm"]
    A = [geo.audio_of(2600, 16000, 40 + s) for s in range(3)]
    cuts = (300, 1300, 2600)  # feed 1: 300 samples (a carry, no frame); feed 2: 1000, asked for as -5 / 1000 / 1100; feed 3: the rest

    def run(asked):
        call = geo.FrontEndCall(window, W, 1300, 3, step, stack, rm)
        m = geo.Mirror(3, L, step, stack, rm)
        got = [[] for _ in range(3)]
        for i, (a, b) in enumerate(zip((0,) + cuts, cuts)):
            smp = asked if i == 1 else [b - a] * 3
            chunks = [x[a:b] for x in A]
            if i == 1:  # what the slot may consume: nothing in slot 0
                chunks[0] = None
            rows, counts = call.feed(chunks, [int(i == 0)] * 3, [int(i == 2)] * 3, 1, samples=smp, cs=b - a)
            assert counts == m.feed(b - a, smp, [int(i == 0)] * 3, [int(i == 2)] * 3), i
            for s in range(3):
                got[s].append(rows[s])
        return [torch.cat(g) for g in got]

    clamped, plain = run([-5, 1000, 1100]), run([0, 1000, 1000])
    for s in range(3):
        assert clamped[s].shape[0] > 0 and torch.equal(clamped[s], plain[s]), s
    # slot 0 skipped the second chunk: its stream is A[0][:300] ++ A[0][1300:]
    skipped = np.concatenate([A[0][:300], A[0][1300:]])
    top = max(geo.check_rows(clamped[0].numpy(), skipped, window, W, step, stack, 1),
              geo.check_rows(clamped[1].numpy(), A[1], window, W, step, stack, 1),
              geo.check_rows(clamped[2].numpy(), A[2], window, W, step, stack, 1))
    _record("abi clamped samples", max_err=top, bar=geo.BAR)


def test_null_arguments_live_reset_and_finished_slots():
    """One script on two slots.  Slot 0: a feed on the poisoned workspace without a reset; stream A; a reset while A is live with
    carry, held frames and a running mean; stream B with reset / final_chunk NULL, with a feed of chunk_samples = 0 and audio =
    NULL in the middle; finished; a feed that is ignored; B again.  Slot 1: stream C throughout, chunked differently.  B (twice)
    and C are bitwise the one-call rows of a fresh one-slot front end, counts follow the mirror on every feed."""
    window, W = _abi_tables()
    L, step, stack, rm = ABI["L"], ABI["step"], ABI["stack"], ABI["rm"]
    A, B, C = (geo.audio_of(n, 16000, seed) for n, seed in ((2000, 50), (3100, 51), (9000, 52)))
    call = geo.FrontEndCall(window, W, 2000, 2, step, stack, rm)
    m = geo.Mirror(2, L, step, stack, rm)
    z = np.zeros(0, np.float32)
    # (slot 0's chunk, slot 1's chunk, reset, final); cs = 0 where both chunks are empty
    script = [
        (A[:2000], C[:1234], None, None),            # right after begin: every slot is FINISHED, nothing comes out
        (A[:1500], C[:1234], [1, 1], None),          # A: 7 frames, 2 rows, 1 held, 380 carried
        (A[1500:2000], C[1234:1300], None, None),    # A: 4 frames, 5 held, 240 carried, n = 11
        (B[:1700], C[1300:3300], [1, 0], None),      # the reset of the live slot applies before B's samples
        (z, z, None, None),                          # chunk_samples = 0, audio = NULL
        (B[1700:1701], C[3300:3300], None, None),
        (B[1701:3100], C[3300:5000], None, [1, 0]),  # B ends
        (A[:2000], C[5000:7000], None, None),        # slot 0 is finished: ignored
        (B[:2000], C[7000:7001], [1, 0], None),      # B again, between two starts
        (B[2000:3100], C[7001:9000], None, [1, 1]),
    ]
    got = {"ignored": [], "B1": [], "B2": [], "C": []}
    stage = ["ignored", "A", "A", "B1", "B1", "B1", "B1", "ignored", "B2", "B2"]
    for i, (x0, x1, reset, final) in enumerate(script):
        rows, counts = call.feed([x0, x1], reset, final, 1)
        assert counts == m.feed(max(len(x0), len(x1)), [len(x0), len(x1)], reset, final), i
        got.setdefault(stage[i], []).append(rows[0])
        if i:
            got["C"].append(rows[1])
        else:
            assert counts == [0, 0]
        if i == 4:
            assert counts == [0, 0]
    assert sum(r.shape[0] for r in got["ignored"]) == 0 and m.trace[0][2]["h0"] + m.trace[0][2]["nf"] == 5 and m.c[0] == 0
    wantB = _one_call(window, W, step, stack, rm, 1, B)
    wantC = _one_call(window, W, step, stack, rm, 1, C)
    assert wantB.shape[0] == (1 + (3100 - L) // step) // stack
    assert torch.equal(torch.cat(got["B1"]), wantB) and torch.equal(torch.cat(got["B2"]), wantB)
    assert torch.equal(torch.cat(got["C"]), wantC)
    top = max(geo.check_rows(wantB.numpy(), B, window, W, step, stack, 1), geo.check_rows(wantC.numpy(), C, window, W, step, stack, 1))
    _record("abi null arguments, live reset, finished slot", max_err=top, bar=geo.BAR)


def test_a_feed_beyond_the_limits_is_refused_before_anything_runs():
    window, W = _abi_tables()
    call = geo.FrontEndCall(window, W, 500, 1, ABI["step"])
    audio = geo.exact(np.zeros((1, 501), np.float32), DEV)
    smp = torch.zeros(1, dtype=torch.int32, device=DEV)
    args = (smp.data_ptr(), None, None, 1, call.rows.data_ptr(), call.counts.data_ptr(), *call.shape, call.ws.data_ptr(), call.opts)
    assert call.lib.compute_rnnt_frontend_feed(audio.data_ptr(), 501, *args) == INVALID_VALUE  # chunk_samples > max_chunk_samples
    assert call.lib.compute_rnnt_frontend_feed(None, 500, *args) == INVALID_VALUE              # audio NULL with samples to read
    torch.cuda.synchronize()
    assert int(call.counts[0]) == -1  # (still the poison: nothing ran)


# ---------------------------------------------------------------------------------------------
# 7. invariance where it has not been shown: 48 kHz (nfft 2048) and M = 160, through StreamingFrontEnd
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sr,hp", [("48 kHz nfft 2048", 48000, fc.hparams()), ("M 160", 16000, fc.hparams(mel_bins=160))])
def test_chunking_invariance_at_nfft_2048_and_at_160_mel_bins(name, sr, hp):
    audio = fc.signal(0.5, sr, seed=13)
    L, S = int(round(sr * hp.frame_length)), int(round(sr * hp.frame_step))
    ref, c0, d0, fe = fc.one_call(audio, hp, sr, 2, "running", DEV)
    assert fe.engine and fe.route == "engine" and fe.nfft == geo.nfft_of(L) == (2048 if sr == 48000 else 512)
    frames = 1 + (len(audio) - L) // S
    assert c0 == d0 == [frames // 3] and ref.shape == (frames // 3, hp.mel_bins * 3)
    x64, floor = fc.raw_log_mel64(audio, sr, hp)
    live = np.setdiff1d(np.arange(hp.mel_bins), geo.empty_filters(fe.mel_w.cpu().numpy()))
    live = np.concatenate([live + i * hp.mel_bins for i in range(3)])
    err = np.abs(ref.numpy() - fc.stacked(fc.running64(x64), 3))[:, live].max()
    assert err < fc.BAR
    chunks = fc.ragged_chunks(len(audio), seed=5, step=S)
    want = fc.expected_counts(chunks, L, S, 3, 2)
    for kw in (dict(slots=3, slot=1, neighbours=True), dict(slots=3, slot=1, neighbours=True, restart=True)):
        rows, counts, dev_counts, fe = fc.feed_stream(audio, chunks, hp, sr, 2, "running", DEV, max_chunk=3000, **kw)
        assert fe.engine
        assert counts == dev_counts == want, (kw, counts, dev_counts, want)
        assert torch.equal(rows, ref), kw
    _record(f"invariance {name}", max_err=err, bar=fc.BAR, feeds=len(chunks))
