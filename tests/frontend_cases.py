"""Shared by tests/test_stream_frontend.py (CPU) and tests/test_stream_frontend_gpu.py: the test signals, the float64
restatement of the streaming front end's definitions (a framing loop + np.fft + oracle.features_oracle.mel_matrix), the
chunkings and the drivers that feed one stream through a StreamingFrontEnd in different slots."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import features_oracle as fo
from rnnt_speech_recognition_amd import features

BAR = 2e-3  # the project's bar for float32 log-mel against a float64 restatement (tests/test_frontend.py:22)


def hparams(mel_bins=80, frame_length=0.025, frame_step=0.01, stack=3, lo=125.0, hi=7600.0):
    return SimpleNamespace(mel_bins=mel_bins, frame_length=frame_length, frame_step=frame_step, hertz_low=lo, hertz_high=hi,
                           downsample_factor=stack)


def signal(seconds, sr=16000, seed=0, tone=440.0):
    """The class of signal tests/test_frontend.py uses: 0.3 sin + 0.1 N(0, 1)."""
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * sr)) / sr
    return (0.3 * np.sin(2 * np.pi * tone * t) + 0.1 * rng.normal(size=t.size)).astype(np.float32)


def raw_log_mel64(audio, sr, hp):
    """x = log(mel + 1e-6) of every frame in float64 -> ([frames, mel_bins], the smallest mel energy)."""
    audio = np.asarray(audio, np.float64)
    L, S = int(round(sr * hp.frame_length)), int(round(sr * hp.frame_step))
    nfft = 1
    while nfft < L:
        nfft *= 2
    win = np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * i / L) for i in range(L)])
    n = 0 if len(audio) < L else 1 + (len(audio) - L) // S
    mag = np.zeros((n, nfft // 2 + 1))
    for i in range(n):
        mag[i] = np.abs(np.fft.rfft(audio[i * S: i * S + L] * win, n=nfft))
    mel = mag @ fo.mel_matrix(hp.mel_bins, nfft // 2 + 1, float(sr), hp.hertz_low, hp.hertz_high)
    return np.log(mel + 1e-6), (mel.min() if n else np.inf)


def running64(x):
    """y_i = x_i - (mean(x_0 ... x_i) + 1e-8), per bin, in float64."""
    n = np.arange(1, x.shape[0] + 1)[:, None]
    return x - (np.cumsum(x, axis=0) / n + 1e-8)


def stacked(frames, stack):
    t = (frames.shape[0] // stack) * stack
    return frames[:t].reshape(-1, frames.shape[1] * stack)


def even_chunks(n, size):
    return [min(size, n - p) for p in range(0, n, size)]


def ragged_chunks(n, seed=7, step=160):
    """Chunks of 0 ... 3000 samples that sum to n: zero-sample feeds, single samples and chunks shorter than a step included."""
    rng = np.random.default_rng(seed)
    head = [0, 1, step - 1, 37, 3000, 0, step, step + 1, 5, 2999]
    out, left = [], n
    for c in head:
        c = min(c, left)
        out.append(c)
        left -= c
    while left > 0:
        c = int(min(rng.integers(0, 3001), left))
        out.append(c)
        left -= c
    assert sum(out) == n and 0 in out and max(out) <= 3000
    return out


def expected_counts(chunks, L, S, stack, rm):
    """The emitted row counts from the sample counts alone (the issue's integer rule), final = the last chunk."""
    c = h = 0
    out = []
    for i, k in enumerate(chunks):
        avail = c + k
        nf = 0 if avail < L else 1 + (avail - L) // S
        c = avail - nf * S
        if i + 1 == len(chunks):
            out.append((h + nf) // stack)
        else:
            out.append(((h + nf) // (stack * rm)) * rm)
            h = (h + nf) % (stack * rm)
    return out


def feed_stream(audio, chunks, hp, sr, rm, norm, device, slots=1, slot=0, neighbours=False, restart=False, engine=None,
                max_chunk=None):
    """One stream through slot `slot` of a `slots`-slot front end -> (rows [R, F] on the CPU, per-feed host counts, per-feed
    device counts, the front end).  neighbours: every other slot carries its own live stream with its own ragged traffic.
    restart: the slot first holds another stream for a few feeds and is started again without having finished it."""
    rng = np.random.default_rng(99)
    fe = features.StreamingFrontEnd(hp, sr, slots, max_chunk or max(1, max(chunks)), rm, norm, device=device, engine=engine)
    others = [s for s in range(slots) if s != slot] if neighbours else []
    fe.start(others)
    if restart:
        fe.start([slot])
        for n in (700, 1, 333):
            au = torch.tensor(rng.normal(size=(slots, n)).astype(np.float32))
            fe.feed(au.to(device), [n] * slots if neighbours else [n if s == slot else 0 for s in range(slots)], [False] * slots)
    fe.start([slot])
    audio = torch.as_tensor(audio)
    got, counts, dev_counts, pos = [], [], [], 0
    for i, n in enumerate(chunks):
        k = [int(rng.integers(0, 2001)) if s in others else 0 for s in range(slots)]
        k[slot] = n
        N = max(k)
        au = torch.tensor(rng.normal(size=(slots, N)).astype(np.float32) * 0.2)
        au[slot, :n] = audio[pos: pos + n]
        fin = [False] * slots
        fin[slot] = i + 1 == len(chunks)
        rows, cnt = fe.feed(au.to(device), k, fin)
        assert rows.shape[0] == slots and rows.shape[2] == fe.F and rows.shape[1] == max(cnt) <= fe.max_rows
        assert not rows[slot, cnt[slot]:].any()  # rows past the count are zeros
        got.append(rows[slot, : cnt[slot]].cpu())
        counts.append(cnt[slot])
        dev_counts.append(int(fe.row_counts[slot]))
        pos += n
    return torch.cat(got), counts, dev_counts, fe


def one_call(audio, hp, sr, rm, norm, device, engine=None):
    return feed_stream(audio, [len(audio)], hp, sr, rm, norm, device, engine=engine)


def check_chunking_invariance(device, rm, engine=None):
    """One stream of about 1.2 s: one call, 1024-sample chunks and ragged chunks; alone, in slot 5 of 8 beside live streams, and
    in a restarted slot.  Rows, total and per-feed counts are bitwise equal; counts follow the integer rule."""
    sr, hp = 16000, hparams()
    audio = signal(1.2, sr, seed=3)
    L, S, stack = 400, 160, hp.downsample_factor
    frames = 1 + (len(audio) - L) // S
    ref, c0, d0, fe = one_call(audio, hp, sr, rm, "running", device, engine)
    assert (device.type != "cuda" or engine is False) or fe.engine
    assert c0 == d0 == [frames // stack] and ref.shape == (frames // stack, hp.mel_bins * stack)
    for chunks in (even_chunks(len(audio), 1024), ragged_chunks(len(audio))):
        want = expected_counts(chunks, L, S, stack, rm)
        assert sum(want) == frames // stack and all(c % rm == 0 for c in want[:-1])
        for kw in (dict(), dict(slots=8, slot=5, neighbours=True), dict(slots=8, slot=5, neighbours=True, restart=True),
                   dict(slots=2, slot=1, restart=True)):
            rows, counts, dev_counts, _ = feed_stream(audio, chunks, hp, sr, rm, "running", device, engine=engine, max_chunk=3000,
                                                      **kw)
            assert counts == want and dev_counts == want, (kw, counts, dev_counts, want)
            assert rows.shape == ref.shape and torch.equal(rows, ref), (kw, float((rows - ref).abs().max()))


def check_parity(device, engine=None):
    """-> the measured maxima (none vs restatement, none minus mean vs the oracle's log_mel, running vs restatement)."""
    sr, hp = 16000, hparams()
    audio = signal(0.73, sr, seed=0)
    x64, floor = raw_log_mel64(audio, sr, hp)
    assert floor > 1e-3  # the log does not amplify float32 noise
    rows, _, _, fe = one_call(audio, hp, sr, 1, "none", device, engine)
    d_none = np.abs(rows.numpy() - stacked(x64, 3)).max()
    # tie to the existing oracle: the frames minus their per-bin mean (+1e-8) are its log_mel
    hp1 = hparams(stack=1)
    frames, _, _, _ = one_call(audio, hp1, sr, 1, "none", device, engine)
    frames = frames.numpy().astype(np.float64)
    d_oracle = np.abs(frames - (frames.mean(axis=0) + 1e-8) - fo.log_mel(audio, sr)).max()
    run, _, _, _ = one_call(audio, hp, sr, 1, "running", device, engine)
    d_run = np.abs(run.numpy() - stacked(running64(x64), 3)).max()
    print(f"front-end parity on {device} ({fe.route}): none {d_none:.3e}  oracle {d_oracle:.3e}  running {d_run:.3e}")
    assert rows.shape == stacked(x64, 3).shape and frames.shape == x64.shape
    assert d_none < BAR and d_oracle < BAR and d_run < BAR
    return d_none, d_oracle, d_run


def check_zero_audio(device, engine=None):
    hp = hparams()
    rows, counts, _, _ = one_call(np.zeros(8000, np.float32), hp, 16000, 1, "none", device, engine)
    assert counts == [(1 + (8000 - 400) // 160) // 3]
    assert torch.equal(rows, torch.full_like(rows, float(np.float32(np.log(1e-6)))))


def check_state_machine(device, engine=None):
    sr, hp = 16000, hparams()
    audio = signal(0.6, sr, seed=5)
    n = len(audio)
    ref, _, _, _ = one_call(audio, hp, sr, 2, "running", device, engine)
    fe = features.StreamingFrontEnd(hp, sr, 3, n, 2, "running", device=device, engine=engine)
    au = torch.tensor(np.stack([audio, signal(0.6, sr, seed=6), audio])).to(device)
    # every slot begins finished: a feed is ignored
    rows, counts = fe.feed(au, [n, n, n], [False] * 3)
    assert counts == [0, 0, 0] and rows.shape[1] == 0
    # a reset with samples in the same call applies first
    fe.start([0])
    rows, counts = fe.feed(au, [n, n, n], [True, False, False])
    assert counts == [ref.shape[0], 0, 0] and torch.equal(rows[0].cpu(), ref) and [int(v) for v in fe.row_counts] == counts
    # finished again: ignored until the next start; then the same stream gives the same rows, beside a neighbour
    rows, counts = fe.feed(au, [n, n, n], [False] * 3)
    assert counts == [0, 0, 0]
    fe.start([1, 2])
    rows, counts = fe.feed(au, [n, 100, n], [True, False, True])
    assert counts == [0, 0, ref.shape[0]] and torch.equal(rows[2].cpu(), ref) and not rows[:2].any()
    # a stream shorter than one frame gives no rows
    rows, counts, dev_counts, _ = feed_stream(audio[:399], [100, 299], hp, sr, 1, "running", device, engine=engine)
    assert counts == dev_counts == [0, 0] and rows.shape[0] == 0


def check_other_shapes(device, engine=None):
    """frame_step == frame_length, and nfft 256 / 1024 (8 kHz / 32 kHz): parity with the restatement, and chunked == one call."""
    out = {}
    for name, sr, hp in (("S == L", 16000, hparams(frame_step=0.025)), ("nfft 256", 8000, hparams(mel_bins=32, hi=3800.0)),
                         ("nfft 1024", 32000, hparams())):
        audio = signal(0.5, sr, seed=11)
        L, S = int(round(sr * hp.frame_length)), int(round(sr * hp.frame_step))
        x64, floor = raw_log_mel64(audio, sr, hp)
        assert floor > 1e-3, name
        ref, c0, _, fe = one_call(audio, hp, sr, 2, "running", device, engine)
        assert fe.nfft == {"S == L": 512, "nfft 256": 256, "nfft 1024": 1024}[name]
        assert (device.type != "cuda" or engine is False) or fe.engine
        assert c0 == [x64.shape[0] // 3]
        out[name] = np.abs(ref.numpy() - stacked(running64(x64), 3)).max()
        assert out[name] < BAR, (name, out[name])
        chunks = ragged_chunks(len(audio), seed=2, step=S)
        rows, counts, dev_counts, _ = feed_stream(audio, chunks, hp, sr, 2, "running", device, slots=3, slot=1, neighbours=True,
                                                  engine=engine, max_chunk=3000)
        assert counts == dev_counts == expected_counts(chunks, L, S, 3, 2), name
        assert torch.equal(rows, ref), name
    print(f"front-end parity on {device}, other shapes: " + "  ".join(f"{k} {v:.3e}" for k, v in out.items()))
