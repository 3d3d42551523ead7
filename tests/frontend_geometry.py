"""The launch geometry of the streaming log-mel front end (csrc/frontend_kernels.hip), restated in plain Python, and the cases
that reach each corner of it.  Shared by tests/test_frontend_geometry.py (CPU) and tests/test_frontend_geometry_gpu.py.

The constants are copied from the .hip file (the CPU test compares the copies with the source).  The helpers only say WHICH
geometry a shape reaches: the FFT size, the frame tiles of a feed, the trips of the two mel-bin loops, the LDS of an
instantiation.  The numerical reference is log_mel64 / rows64: a float64 restatement of include/rnnt.h's definitions (frames,
np.fft.rfft, |X| @ W, log(+1e-6), the running mean, stacking) for an ARBITRARY window and mel matrix, both taken as the float32
values the device gets.  Mirror is the header's integer state machine per slot, with the rules only the C ABI can reach.
FrontEndCall drives compute_rnnt_frontend_begin / _feed with every buffer poisoned.  Nothing of the code under test is imported
by the reference; features.linear_to_mel_weight_matrix only makes the standard INPUT matrix."""
import math

import numpy as np

from tests import frontend_cases as fc

# ---- constants (name in frontend_kernels.hip -> value)
CONSTANTS = {"kFeWaves": 4, "kFeTile": 16, "kFeEmitThreads": 128, "kFeMaxLen": 2048}
WAVES, TILE, EMIT_THREADS, MAX_LEN = (CONSTANTS[k] for k in ("kFeWaves", "kFeTile", "kFeEmitThreads", "kFeMaxLen"))
LANES = 64
LDS_LIMIT = 160 * 1024  # bytes of LDS a gfx950 workgroup can have
BAR = fc.BAR
LOG_FLOOR = float(np.float32(np.log(1e-6)))  # x of an empty filter
FLOOR = 1e-3  # the project's condition for BAR: no mel energy (no |X_k| of the spectrum group) of the reference below it


# ---- which geometry a shape reaches
def nfft_of(L):
    n = 1
    while n < L:
        n *= 2
    return n


def frames_of(avail, L, step):
    return 0 if avail < L else 1 + (avail - L) // step


def tiles_of(nf):
    """Workgroups of fe_frames_kernel that do work for a slot completing nf frames."""
    return -(-nf // TILE)


def grid_tiles(cs, step):
    """Frame tiles launched per slot for a call of chunk_samples = cs."""
    return tiles_of(1 + (cs - 1) // step) if cs >= 1 else 0


def band_trips(M):
    """Trips of the band-sum loop (j = lane; j < M; j += 64)."""
    return -(-M // LANES)


def emit_trips(M):
    """Trips of the emit kernel's loop (b = tid; b < M; b += 128)."""
    return -(-M // EMIT_THREADS)


def lds_bytes(N):
    """Static LDS of fe_frames_kernel<N>: the twiddles [N] float2, and per wave re[N], im[N], mag[N/2 + 1]."""
    return 8 * N + WAVES * (4 * N + 4 * N + 4 * (N // 2 + 1))


def max_rows(K, step, stack, rm):
    return (stack * rm - 1 + 1 + (K - 1) // step) // stack


def workspace_bytes(K, S, L, step, M, stack, rm):
    """make_fe_layout: window, the packed matrix, the bands, the twiddles, the state words, msum, carry, held frames, x."""
    a256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
    N, G, NF = nfft_of(L), stack * rm, 1 + (K - 1) // step
    nbp = (N // 2 + 1 + 3) // 4 * 4
    return (a256(4 * L) + a256(4 * M * nbp) + 2 * a256(4 * M) + a256(8 * N) + a256(16 * S) + a256(4 * S * M) + a256(4 * S * L)
            + a256(4 * S * G * M) + a256(4 * S * NF * M))


# ---- inputs
def hann(L):
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * i / L) for i in range(L)]).astype(np.float32)


def skewed_window(L):
    """A window that is neither Hann nor symmetric (Hann times a ramp 0.75 ... 1.25): the kernels must use the window they are
    given, sample for sample."""
    return (hann(L).astype(np.float64) * (0.75 + 0.5 * np.arange(L) / L)).astype(np.float32)


def mel_weights(M, nb, sr, lo, hi):
    """The standard matrix, float32 [nb, M], as StreamingFrontEnd hands it to the device."""
    from rnnt_speech_recognition_amd import features

    return features.linear_to_mel_weight_matrix(M, nb, float(sr), lo, hi).numpy()


def bin_picker(nb, M, off):
    """W[k, j] = 1 iff k == j + off: 'filter' j is spectrum bin j + off alone."""
    W = np.zeros((nb, M), np.float32)
    j = np.arange(M)
    j = j[j + off < nb]
    W[j + off, j] = 1.0
    return W


def empty_filters(W):
    return np.flatnonzero(~(np.asarray(W) != 0).any(axis=0))


def audio_of(n, sr, seed, tone=440.0, tone2=None):
    """fc.signal's class (0.3 sin + 0.1 N(0, 1)) for a sample count; tone2 adds a second tone of amplitude 0.2."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = 0.3 * np.sin(2 * np.pi * tone * t) + 0.1 * rng.normal(size=t.size)
    if tone2:
        x = x + 0.2 * np.sin(2 * np.pi * tone2 * t)
    return x.astype(np.float32)


# ---- the float64 restatement
def log_mel64(audio, window, W, step):
    """-> (x = log(mel + 1e-6) [frames, M], mel [frames, M]) in float64; window [L] and W [nfft/2 + 1, M] widened from float32."""
    a = np.asarray(audio, np.float32).astype(np.float64)
    w = np.asarray(window, np.float32).astype(np.float64)
    W = np.asarray(W, np.float32).astype(np.float64)
    L, N = len(w), nfft_of(len(w))
    assert W.shape[0] == N // 2 + 1
    n = frames_of(len(a), L, step)
    mag = np.zeros((n, N // 2 + 1))
    for i in range(n):
        mag[i] = np.abs(np.fft.rfft(a[i * step: i * step + L] * w, n=N))
    mel = mag @ W
    return np.log(mel + 1e-6), mel


def rows64(audio, window, W, step, stack, norm):
    x, _ = log_mel64(audio, window, W, step)
    return fc.stacked(fc.running64(x) if norm else x, stack)


def floor_of(audio, window, W, step):
    """The smallest float64 mel energy over the non-empty filters (inf without frames)."""
    _, mel = log_mel64(audio, window, W, step)
    live = np.setdiff1d(np.arange(W.shape[1]), empty_filters(W))
    return float(mel[:, live].min()) if mel.shape[0] and live.size else math.inf


# ---- the integer state machine of include/rnnt.h, per slot
class Mirror:
    def __init__(self, S, L, step, stack, rm):
        self.S, self.L, self.step, self.stack, self.rm, self.G = S, L, step, stack, rm, stack * rm
        self.c, self.h, self.fin = [0] * S, [0] * S, [True] * S  # begin leaves every slot FINISHED
        self.trace = [[] for _ in range(S)]  # per slot and feed: dict(live, h0, nf, count, final)

    def feed(self, cs, samples, reset=None, final=None):
        counts = []
        for s in range(self.S):
            if reset is not None and reset[s]:  # before the call's samples are taken
                self.c[s] = self.h[s] = 0
                self.fin[s] = False
            live = not self.fin[s]
            k = min(max(int(samples[s]), 0), cs) if live else 0  # clamped into 0 ... chunk_samples
            fin = live and final is not None and bool(final[s])
            avail = self.c[s] + k
            nf = frames_of(avail, self.L, self.step) if live else 0
            h0 = self.h[s]
            total = h0 + nf
            count = 0 if not live else (total // self.stack if fin else (total // self.G) * self.rm)
            if live:
                self.c[s] = 0 if fin else avail - nf * self.step
                self.h[s] = 0 if fin else total - count * self.stack
                self.fin[s] = fin
            self.trace[s].append(dict(live=live, h0=h0, nf=nf, count=count, final=fin))
            counts.append(count)
        return counts


# ---- the C ABI with every buffer poisoned
def exact(x, dev):
    """x at the head of a buffer whose tail is NaN: the tensor ends where its data ends (tests/test_tdt_joint_gpu.py _exact)."""
    import torch

    x = np.ascontiguousarray(x, np.float32)
    buf = torch.full((x.size + 4096,), float("nan"), device=dev)
    buf[: x.size] = torch.as_tensor(x.ravel(), device=dev)
    return buf[: x.size].view(*x.shape)


class FrontEndCall:
    """One front end through the C ABI.  The workspace, rows_out and row_counts are 0xFF bytes before begin, rows and counts
    again before every feed; the window and the mel matrix sit exactly to size in front of NaN, and so does the audio, whose
    rows are NaN beyond samples[s]."""

    def __init__(self, window, W, K, S, step, stack=1, rm=1, dev="cuda:0"):
        import torch
        from rnnt_speech_recognition_amd import _lib

        self.torch, self._lib, self.lib, self.dev = torch, _lib, _lib.load(), torch.device(dev)
        self.L, (self.nb, self.M) = len(window), W.shape
        assert self.nb == nfft_of(self.L) // 2 + 1
        self.K, self.S, self.step, self.stack, self.rm = K, S, step, stack, rm
        self.shape = (K, S, self.L, step, self.M, stack, rm)
        self.max_rows, self.F = max_rows(K, step, stack, rm), self.M * stack
        self.ws = torch.full((_lib.frontend_workspace_bytes(*self.shape),), 0xFF, dtype=torch.uint8, device=self.dev)
        self.rows = torch.empty(S, self.max_rows, self.F, dtype=torch.float32, device=self.dev)
        self.counts = torch.empty(S, dtype=torch.int32, device=self.dev)
        self._poison()
        self.window, self.mel = exact(window, self.dev), exact(W, self.dev)
        self.opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, 1, 1)
        _lib.check(self.lib.compute_rnnt_frontend_begin(self.window.data_ptr(), self.mel.data_ptr(), *self.shape, self.ws.data_ptr(),
                                                        self.opts), "compute_rnnt_frontend_begin")

    def _poison(self):
        self.rows.view(self.torch.uint8).fill_(0xFF)
        self.counts.view(self.torch.uint8).fill_(0xFF)

    def _i32(self, v):
        return None if v is None else self.torch.tensor([int(x) for x in v], dtype=self.torch.int32, device=self.dev)

    def feed(self, chunks, reset=None, final=None, norm=1, samples=None, cs=None):
        """chunks: per slot the samples it consumes (an array, or None for none).  samples / cs override what the call says
        (default: the chunks' lengths and the longest of them).  -> (per slot its rows [count, F] on the CPU, counts)."""
        torch = self.torch
        lens = [0 if c is None else len(c) for c in chunks]
        cs = max(lens) if cs is None else cs
        host = np.full((self.S, cs), np.nan, np.float32)
        for s, c in enumerate(chunks):
            host[s, : lens[s]] = 0 if c is None else c
        audio = exact(host, self.dev) if cs > 0 else None
        smp, rst, fin = self._i32(lens if samples is None else samples), self._i32(reset), self._i32(final)
        self._poison()
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        st = self.lib.compute_rnnt_frontend_feed(ptr(audio), cs, smp.data_ptr(), ptr(rst), ptr(fin), int(norm), self.rows.data_ptr(),
                                                 self.counts.data_ptr(), *self.shape, self.ws.data_ptr(), self.opts)
        self._lib.check(st, "compute_rnnt_frontend_feed")
        torch.cuda.synchronize()
        rows, counts = self.rows.cpu(), [int(v) for v in self.counts.cpu()]
        assert all(0 <= n <= self.max_rows for n in counts), counts  # no poison left in row_counts
        assert bool(torch.isfinite(rows).all())                      # nor in rows_out, and no NaN was read from past an input
        for s, n in enumerate(counts):
            assert not rows[s, n:].any(), s                          # rows past a slot's count are exact zeros out to max_rows
        return [rows[s, :n].clone() for s, n in enumerate(counts)], counts


# ---- the cases.  A case is one front end and, per live slot, one stream with its chunking: feed i gives every slot its i-th
# chunk (nothing once it has run out), a slot is reset with its first chunk and final with its last; slots without a stream
# stay FINISHED.  `reach` is the geometry the case is named for (tests/test_frontend_geometry.py asserts every entry).
def chunks_for_frames(frames, L, step, extra=0):
    """Chunk sizes that complete exactly frames[i] frames in feed i of a fresh stream."""
    out, c = [], 0
    for i, nf in enumerate(frames):
        if nf == 0:
            k = min(3, L - 1 - c)
        else:
            avail = L + (nf - 1) * step + (extra + i) % step
            k = avail - c
        c = c + k - nf * step
        out.append(k)
    return out


def climb(stack, rm):
    """Frames per feed: 0, 1 or a few at a time until G - 1 are held, a feed that emits nothing, one that crosses G by several
    groups, two small ones, and a final feed that leaves a partial group."""
    G, fr, h = stack * rm, [], 0
    while h < G - 1:
        nf = min((0, 1, 3, 2, 5)[len(fr) % 5], G - 1 - h)
        fr.append(nf)
        h += nf
    fr += [0, 2 * G + 2]
    h = (h + 2 * G + 2) % G
    fr += [0, 1]
    h = (h + 1) % G
    return fr + [2 * stack + 1 - h]


def _case(sr, L, step, M, streams, stack=1, rm=1, lo=125.0, hi=None, S=None, norms=(0, 1), **reach):
    """streams: slot -> (seed, chunks)."""
    S = S or max(streams) + 1
    K = max(max(ch) for _, ch in streams.values())
    return dict(sr=sr, L=L, step=step, M=M, stack=stack, rm=rm, lo=lo, hi=hi or 0.475 * sr, S=S, K=max(K, 1), streams=streams,
                norms=norms, reach=reach)


def _width(M):
    return _case(16000, 400, 160, M, {0: (M, [4000])}, nfft=512, tiles=[2], band=band_trips(M), emit=emit_trips(M),
                 empty={127: 1, 128: 1, 129: 1, 160: 3}.get(M, 0))  # (counted on the CPU: filters narrower than a bin)


def _stacking(stack, rm):
    L, step = 200, 80
    short = [min(1, stack - 1), 0]  # total < stack at its final feed: 0 rows
    return _case(8000, L, step, 5, {0: (1, chunks_for_frames(short, L, step)), 1: (2, chunks_for_frames(climb(stack, rm), L, step, 7))},
                 stack=stack, rm=rm, S=3, norms=(1,), nfft=256, held=stack * rm - 1)


_TILE_FRAMES = (0, 1, 15, 16, 17, 33)
CASES = {f"width_M{M}": _width(M) for M in (1, 63, 64, 65, 127, 128, 129, 160)}
CASES["width_M1024_nfft2048"] = _case(16000, 2048, 512, 1024, {0: (11, [8000])}, hi=7600.0, nfft=2048, tiles=[1], band=16, emit=8,
                                      empty=98)
CASES.update({f"stack{a}_rm{b}": _stacking(a, b) for a, b in ((1, 1), (1, 16), (16, 1), (16, 16), (5, 3))})
CASES["tiles_0_1_15_16_17_33"] = _case(
    16000, 400, 160, 40, {s: (20 + s, [399] if nf == 0 else [400 + (nf - 1) * 160 + 11 * s]) for s, nf in enumerate(_TILE_FRAMES)},
    norms=(1,), nfft=512, tiles=[tiles_of(nf) for nf in _TILE_FRAMES], grid=3)
CASES["step1_L129"] = _case(8000, 129, 1, 20, {0: (5, [128, 1, 1, 7, 0, 2893])}, norms=(1,), nfft=256, frames=2902)
CASES["step_eq_len_2048"] = _case(16000, 2048, 2048, 40, {0: (6, [2047, 1, 2 * 2048 + 5, 0, 2048 + 300, 1800])}, nfft=2048,
                                  frames=5)
CASES["chunk1_L129"] = _case(8000, 129, 2, 20, {0: (7, [1] * 140)}, stack=2, norms=(1,), nfft=256, frames=6, first_frame_feed=129)
CASES["slots1024"] = _case(16000, 400, 160, 20, {s: (300 + s, [600 - s // 64, 300 + s // 64]) for s in range(0, 1024, 64)},
                           S=1024, norms=(1,), nfft=512, live=16)

# the spectrum group: (nfft, L) -> seed; 17 frames in one feed, W picks single bins
SPECTRUM_STEP, SPECTRUM_FRAMES = 53, 17
SPECTRUM = {(N, L): 0 for N in (256, 512, 1024, 2048) for L in (N, N // 2 + 1)}
SPECTRUM[(256, 129)] = 1  # (the first seed whose float64 reference has every |X_k| above FLOOR; seed 0 gives 1.1e-4 here)


def spectrum_audio(N, L):
    n = L + (SPECTRUM_FRAMES - 1) * SPECTRUM_STEP
    return audio_of(n, 16000, SPECTRUM[(N, L)], tone=440.0, tone2=4960.0)


def spectrum_window(L):
    return skewed_window(L)


def spectrum_pickers(N):
    """The begins that together cover DC ... Nyquist: (M, off)."""
    nb = N // 2 + 1
    return [(nb, 0)] if N <= 1024 else [(1024, 0), (1024, 1)]


def tables(c):
    return hann(c["L"]), mel_weights(c["M"], nfft_of(c["L"]) // 2 + 1, c["sr"], c["lo"], c["hi"])


def stream_audio(c, slot):
    seed, chunks = c["streams"][slot]
    return audio_of(sum(chunks), c["sr"], seed)


def feeds_of(c):
    """-> per feed (chunks per slot (arrays or None), reset [S], final [S])."""
    S, streams = c["S"], c["streams"]
    audio = {s: stream_audio(c, s) for s in streams}
    out = []
    for i in range(max(len(ch) for _, ch in streams.values())):
        chunks, reset, final = [None] * S, [0] * S, [0] * S
        for s, (_, ch) in streams.items():
            if i < len(ch):
                p = sum(ch[:i])
                chunks[s] = audio[s][p: p + ch[i]]
                reset[s], final[s] = int(i == 0), int(i + 1 == len(ch))
        out.append((chunks, reset, final))
    return out


def mirror_of(c):
    """The mirror after every feed of the case, and the counts per feed."""
    m = Mirror(c["S"], c["L"], c["step"], c["stack"], c["rm"])
    counts = [m.feed(max(len(x) if x is not None else 0 for x in chunks), [0 if x is None else len(x) for x in chunks], reset, final)
              for chunks, reset, final in feeds_of(c)]
    return m, counts


def hparams_of(c):
    return fc.hparams(mel_bins=c["M"], frame_length=c["L"] / c["sr"], frame_step=c["step"] / c["sr"], stack=c["stack"], lo=c["lo"],
                      hi=c["hi"])


def check_rows(got, audio, window, W, step, stack, norm):
    """One stream's rows [R, M * stack] (float32, NumPy) against the restatement -> the largest error over non-empty filters.
    Non-empty filters within BAR; empty filters exactly float32(log(1e-6)) with norm 0, within BAR of the running form with 1."""
    want = rows64(audio, window, W, step, stack, norm)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    M = W.shape[1]
    empty = np.zeros(M, bool)
    empty[empty_filters(W)] = True
    empty = np.tile(empty, stack)
    err = np.abs(got.astype(np.float64) - want)
    if empty.any():
        if norm:
            assert err[:, empty].max() < BAR, err[:, empty].max()
        else:
            assert (got[:, empty] == np.float32(LOG_FLOOR)).all()
    top = float(err[:, ~empty].max()) if (~empty).any() else 0.0
    assert top < BAR, top
    return top
