"""Input side of the path: log-mel front end, text encoding and the 5-tensor training record.

Reference: utils/preprocessing.py:48-94 (compute_mel_spectrograms, downsample_spec), :177-183 (preprocess_text),
:236-296 (preprocess_audio / the record), utils/vocabulary.py:3-6 (character vocabulary), hparams.py:7-12 (front-end
defaults), run_rnnt.py:78-83 (zero-padded batches).  TensorFlow's signal ops are restated from their documented
definitions (tf.signal.stft: periodic Hann window, fft_length = next power of two, no end padding;
tf.signal.linear_to_mel_weight_matrix: HTK mel scale, triangles in the mel domain, DC bin excluded).
TensorFlow is not available in this image, so these are checked against the NumPy restatement in
oracle/features_oracle.py and against closed-form properties, not against TF outputs (parity unpinned, as for the loss).
`make_record` / `padded_batch` produce the five tensors from raw audio + text; the reference's `<name>.tfrecord` files of
those records are read and written by records.py (TFRecord framing, tf.train.Example and TensorProto wire formats,
utils/preprocessing.py:97-161), without TensorFlow.

Runs on whatever device the audio tensor lives on (cuFFT's ROCm counterpart through torch.fft on an MI355X).

StreamingFrontEnd is the CAUSAL counterpart for live audio: chunks of raw samples in, stacked log-mel rows out, for a batch of
slots, with the state kept between feeds (include/rnnt.h, streaming log-mel front end).  Its norm="running" features subtract the
mean of the frames SO FAR, not the per-utterance mean the reference trains on: they are different features, and a model that is
to be streamed this way should be trained on them (running_mean_log_mel gives them for a whole utterance)."""
from __future__ import annotations

import ctypes
import math
from typing import List, Sequence, Tuple

import torch


def _next_pow2(n: int) -> int:
    return 1 << max(0, (int(n) - 1).bit_length())


def hertz_to_mel(f):
    """HTK mel scale used by tf.signal.linear_to_mel_weight_matrix."""
    return 1127.0 * torch.log1p(torch.as_tensor(f, dtype=torch.float64) / 700.0)


def linear_to_mel_weight_matrix(num_mel_bins: int, num_spectrogram_bins: int, sample_rate: float,
                                lower_edge_hertz: float, upper_edge_hertz: float) -> torch.Tensor:
    """[num_spectrogram_bins, num_mel_bins] triangular filterbank (f64 arithmetic, returned as f32)."""
    nyquist = sample_rate / 2.0
    lin = torch.linspace(0.0, nyquist, num_spectrogram_bins, dtype=torch.float64)[1:]  # DC bin left out
    spec_mel = hertz_to_mel(lin)[:, None]
    edges = torch.linspace(float(hertz_to_mel(lower_edge_hertz)), float(hertz_to_mel(upper_edge_hertz)),
                           num_mel_bins + 2, dtype=torch.float64)
    lower, center, upper = edges[:-2][None, :], edges[1:-1][None, :], edges[2:][None, :]
    lower_slopes = (spec_mel - lower) / (center - lower)
    upper_slopes = (upper - spec_mel) / (upper - center)
    w = torch.clamp(torch.minimum(lower_slopes, upper_slopes), min=0.0)
    return torch.cat([torch.zeros(1, num_mel_bins, dtype=torch.float64), w], dim=0).to(torch.float32)


def stft_magnitude(audio: torch.Tensor, frame_length: int, frame_step: int) -> torch.Tensor:
    """|tf.signal.stft(audio, frame_length, frame_step)| : [frames, fft_length/2 + 1]; frames = 1 + (N - L) // step
    (no padding at the end), periodic Hann window, zero-padded to the next power of two."""
    audio = audio.to(torch.float32)
    n = audio.shape[-1]
    if n < frame_length:
        return audio.new_zeros((0, _next_pow2(frame_length) // 2 + 1))
    frames = audio.unfold(-1, frame_length, frame_step)  # [F, L]
    k = torch.arange(frame_length, device=audio.device, dtype=torch.float32)
    window = 0.5 - 0.5 * torch.cos(2.0 * math.pi * k / frame_length)  # periodic
    return torch.fft.rfft(frames * window, n=_next_pow2(frame_length), dim=-1).abs()


def compute_mel_spectrograms(audio_arr: torch.Tensor, sample_rate: int, n_mel_bins: int = 80,
                             frame_length: float = 0.025, frame_step: float = 0.01, hertz_low: float = 125.0,
                             hertz_high: float = 7600.0) -> torch.Tensor:
    """utils/preprocessing.py:48-81: log(mel + 1e-6) minus its per-bin mean over time (+1e-8)."""
    sr = float(sample_rate)
    fl, fs = int(round(sr * frame_length)), int(round(sr * frame_step))
    mag = stft_magnitude(audio_arr, fl, fs)
    mel_w = linear_to_mel_weight_matrix(n_mel_bins, mag.shape[-1], sr, hertz_low, hertz_high).to(mag.device)
    log_mel = torch.log(mag @ mel_w + 1e-6)
    return log_mel - (log_mel.mean(dim=0) + 1e-8)


def downsample_spec(mel_spec: torch.Tensor, n: int = 3) -> torch.Tensor:
    """utils/preprocessing.py:84-94: drop the tail that does not fill a group, stack n consecutive frames."""
    t, f = mel_spec.shape
    t3 = (t // n) * n
    return mel_spec[:t3].reshape(-1, f * n)


def preprocess_audio(audio: torch.Tensor, sample_rate: int, hp) -> torch.Tensor:
    """utils/preprocessing.py:236-253 with the front-end fields of model.HParams."""
    spec = compute_mel_spectrograms(audio, sample_rate, hp.mel_bins, hp.frame_length, hp.frame_step, hp.hertz_low,
                                    hp.hertz_high)
    return downsample_spec(spec, hp.downsample_factor)


# ---- streaming front end ----------------------------------------------------------------------------------------
class StreamingFrontEnd:
    """Log-mel rows from live audio, for `slots` streams at once, fed chunk by chunk (include/rnnt.h, streaming log-mel front
    end).  hp gives mel_bins, frame_length, frame_step, hertz_low, hertz_high and downsample_factor (the frames stacked into a
    row); row_multiple is the encoder's reduction factor: a non-final feed returns a multiple of it, as the streaming decoders
    require.

    start(slots) (re)starts a stream in the given slots (indices, or a bool mask [slots]); every slot begins FINISHED.
    feed(audio [slots, N], samples [slots], final [slots]) -> (rows [slots, R, mel_bins * stack], counts): slot s consumes
    audio[s, :samples[s]]; counts (a host list, from the integer mirror of the state -- nothing is read back) says how many of the
    R = max(counts) rows are the slot's, the others are zeros.  samples and final are host data.  A finished slot ignores feeds
    until its next start.  max_rows bounds R for any feed of up to max_chunk_samples samples.

    norm="running": each frame minus the mean of the stream's frames so far (itself included), per bin, + 1e-8 -- the causal
    counterpart of compute_mel_spectrograms' per-utterance mean; norm="none": the raw log(mel + 1e-6).  Frame i of a stream
    always covers its samples i * step ... i * step + L - 1, and every sum is taken in a fixed order: a stream's rows are bitwise
    independent of how it was chunked, of the slot and of the other slots (on the engine and, among its own runs, in torch).

    On an MI355X this is the ENGINE (compute_rnnt_frontend_begin / _feed: two launches per feed, no host synchronisation).  On
    CPU, with engine=False, or for shapes the kernels do not take (`route` says which and why), the same state machine runs in
    torch: gather, window, rfft, band sum, log, the running sum frame by frame in float32, gathers for rows, held frames and
    carry."""

    NORMS = ("none", "running")

    def __init__(self, hp, sample_rate, slots: int, max_chunk_samples: int, row_multiple: int = 1, norm: str = "running",
                 device=None, engine=None):
        if norm not in self.NORMS:
            raise ValueError(f"norm must be one of {self.NORMS}, got {norm!r}")
        sr = float(sample_rate)
        L, step = int(round(sr * hp.frame_length)), int(round(sr * hp.frame_step))
        S, K, M = int(slots), int(max_chunk_samples), int(hp.mel_bins)
        stack, rm = int(hp.downsample_factor), int(row_multiple)
        if S < 1 or K < 1 or M < 1 or stack < 1 or rm < 1 or L < 1 or step < 1:
            raise ValueError(f"slots, max_chunk_samples, mel_bins, downsample_factor, row_multiple, frame length and step must be "
                             f">= 1, got {S}, {K}, {M}, {stack}, {rm}, {L}, {step}")
        if step > L:
            raise ValueError(f"frame step {step} exceeds the frame length {L}: samples would be skipped")
        self.S, self.K, self.M, self.L, self.step, self.stack, self.rm, self.G = S, K, M, L, step, stack, rm, stack * rm
        self.norm, self.nfft = norm, _next_pow2(L)
        self.F = M * stack
        self.NF = 1 + (K - 1) // step  # frames one feed can complete
        self.max_rows = (self.G - 1 + self.NF) // stack
        dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.dev = dev
        nb = self.nfft // 2 + 1
        k = torch.arange(L, dtype=torch.float64)
        self.window = (0.5 - 0.5 * torch.cos(2.0 * math.pi * k / L)).to(torch.float32).to(dev)  # float64, rounded once
        self.mel_w = linear_to_mel_weight_matrix(M, nb, sr, hp.hertz_low, hp.hertz_high).contiguous().to(dev)
        self._c, self._n, self._h, self._fin = [0] * S, [0] * S, [0] * S, [True] * S  # the integer mirror of the state
        self._pending = [False] * S
        self.row_counts = None
        self.engine, self.route = False, "torch: CPU tensors"
        if engine is False:
            self.route = "torch: asked for (engine=False)"
        elif dev.type == "cuda":
            from . import _lib

            n = ctypes.c_size_t(0)
            ok = _lib.load().get_rnnt_frontend_workspace_size(K, S, L, step, M, stack, rm, n) == _lib.STATUS_SUCCESS
            self.engine = ok
            self.route = "engine" if ok else "torch: a shape the kernels do not take"
        if engine is True and not self.engine:
            raise RuntimeError(f"StreamingFrontEnd: the engine was asked for but cannot run ({self.route})")
        if self.engine:
            from . import _lib
            from .joint import _workspace

            with torch.cuda.device(dev):
                self._ws = _workspace(None, int(n.value), dev)  # (a front end begins once: always a fresh one)
                self._opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, 1, 1)
                st = _lib.load().compute_rnnt_frontend_begin(self.window.data_ptr(), self.mel_w.data_ptr(), K, S, L, step, M, stack,
                                                             rm, self._ws.data_ptr(), self._opts)
            _lib.check(st, "compute_rnnt_frontend_begin")
            return
        # the torch route's tables and state
        W = self.mel_w.cpu()
        nz = W != 0
        lo = [int(nz[:, j].nonzero()[0]) if nz[:, j].any() else 0 for j in range(M)]
        hi = [int(nz[:, j].nonzero()[-1]) + 1 if nz[:, j].any() else 0 for j in range(M)]
        width = max(1, max(h - l for l, h in zip(lo, hi)))
        idx = (torch.tensor(lo)[:, None] + torch.arange(width)[None, :])
        inside = idx < torch.tensor(hi)[:, None]
        idx = idx.clamp(max=nb - 1)
        self._bidx = idx.to(dev)                                                                # [M, width] bins of each band
        self._bw = torch.where(inside, W[idx, torch.arange(M)[:, None]], torch.zeros(())).to(dev)  # [M, width] their weights
        self._carry = torch.zeros(S, L, device=dev)
        self._held = torch.zeros(S, self.G, M, device=dev)
        self._msum = torch.zeros(S, M, device=dev)

    # ---- slots
    def _mask(self, slots):
        t = torch.as_tensor(slots)
        if t.dtype == torch.bool:
            if t.numel() != self.S:
                raise ValueError(f"a slot mask must have {self.S} entries, got {t.numel()}")
            return [bool(v) for v in t.reshape(-1).tolist()]
        m = [False] * self.S
        for s in t.reshape(-1).tolist():
            if not 0 <= int(s) < self.S:
                raise ValueError(f"slot {s} is not in 0 ... {self.S - 1}")
            m[int(s)] = True
        return m

    @torch.no_grad()
    def start(self, slots) -> None:
        m = self._mask(slots)
        for s in range(self.S):
            if m[s]:
                self._c[s] = self._n[s] = self._h[s] = 0
                self._fin[s] = False
                self._pending[s] = True  # (the engine takes the reset with the next feed, before that feed's samples)
        if not self.engine and any(m):
            self._msum[torch.tensor(m, device=self.dev)] = 0.0

    def _check_feed(self, audio, samples, final):
        S = self.S
        if audio.dim() != 2 or audio.shape[0] != S:
            raise ValueError(f"audio must be [{S}, samples], got {tuple(audio.shape)}")
        N = int(audio.shape[1])
        if N > self.K:
            raise ValueError(f"audio has {N} samples per slot; this front end takes at most max_chunk_samples = {self.K}")
        k = [int(v) for v in torch.as_tensor(samples).reshape(-1).tolist()]
        fi = [bool(v) for v in torch.as_tensor(final).reshape(-1).tolist()]
        if len(k) != S or len(fi) != S:
            raise ValueError(f"samples and final must have {S} entries")
        for s in range(S):
            if not 0 <= k[s] <= N:
                raise ValueError(f"samples[{s}] = {k[s]} is not in 0 ... {N}")
        return N, k, fi

    def _plan(self, k, fi):
        """Advance the integer mirror by one feed -> per slot (live, c, k, nf, h, count, final) as they were for this feed."""
        plan = []
        L, step, stack, G = self.L, self.step, self.stack, self.G
        for s in range(self.S):
            live = not self._fin[s]
            c, h = self._c[s], self._h[s]
            ks = k[s] if live else 0
            avail = c + ks
            nf = 0 if (not live or avail < L) else 1 + (avail - L) // step
            fin = live and fi[s]
            total = h + nf
            count = 0 if not live else (total // stack if fin else (total // G) * self.rm)
            plan.append((live, c, ks, nf, h, count, fin))
            if live:
                self._c[s] = 0 if fin else avail - nf * step
                self._h[s] = 0 if fin else total - count * stack
                self._n[s] = 0 if fin else (self._n[s] + nf if self.norm == "running" else self._n[s])
                self._fin[s] = fin
        return plan

    @torch.no_grad()
    def feed(self, audio: torch.Tensor, samples, final):
        N, k, fi = self._check_feed(audio, samples, final)
        n_before = list(self._n)
        plan = self._plan(k, fi)
        counts = [p[5] for p in plan]
        R = max(counts)
        pending, self._pending = self._pending, [False] * self.S
        if not self.engine:
            rows = self._torch_feed(audio, N, plan, n_before, R)
            self.row_counts = torch.tensor(counts, dtype=torch.int32)
            return rows, counts
        from . import _lib
        from .joint import _aligned16, _device_i32

        dev = self.dev
        au = _aligned16(audio.to(device=dev, dtype=torch.float32)) if N > 0 else None
        smp = _device_i32(k, dev)
        rst = _device_i32([int(v) for v in pending], dev) if any(pending) else None
        fin = _device_i32([int(v) for v in fi], dev) if any(fi) else None
        rows = torch.empty(self.S, self.max_rows, self.F, dtype=torch.float32, device=dev)
        cnt = torch.empty(self.S, dtype=torch.int32, device=dev)
        self._args = (au, smp, rst, fin)  # (alive until the launches have read them)
        st = _lib.load().compute_rnnt_frontend_feed(None if au is None else au.data_ptr(), N, smp.data_ptr(),
                                                    None if rst is None else rst.data_ptr(), None if fin is None else fin.data_ptr(),
                                                    int(self.norm == "running"), rows.data_ptr(), cnt.data_ptr(), self.K, self.S,
                                                    self.L, self.step, self.M, self.stack, self.rm, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_frontend_feed")
        self.row_counts = cnt
        return rows[:, :R], counts

    # ---- torch composition
    def _torch_feed(self, audio, N, plan, n_before, R):
        S, L, step, M, G, stack, dev = self.S, self.L, self.step, self.M, self.G, self.stack, self.dev
        ar = torch.arange
        c = torch.tensor([p[1] for p in plan])[:, None]
        nf = torch.tensor([p[3] for p in plan])
        h = torch.tensor([p[4] for p in plan])[:, None]
        live = torch.tensor([p[0] for p in plan])[:, None]
        fin = torch.tensor([p[6] for p in plan])
        NFc = int(nf.max())
        buf = torch.cat([self._carry, audio.to(device=dev, dtype=torch.float32)], dim=1)  # [S, L + N]
        a_of = lambda p: torch.where(p < c, p, L + p - c).clamp(max=L + N - 1)  # noqa: E731  sample p of carry ++ chunk, in buf
        if NFc > 0:
            sig = buf.gather(1, a_of(ar(L - 1 + N)[None, :].expand(S, -1)).to(dev))
            frames = sig.unfold(1, L, step)[:, :NFc]                                    # [S, NFc, L]
            spec = torch.fft.rfft(frames * self.window, n=self.nfft, dim=-1).abs()       # [S, NFc, nb]
            mel = (spec[..., self._bidx] * self._bw).sum(dim=-1)                         # each band on its own, contiguous
            x = torch.log(mel.double() + 1e-6).to(torch.float32)                         # [S, NFc, M]
            if self.norm == "running":
                mask = (ar(NFc)[None, :] < nf[:, None]).to(dev)
                ntab = (torch.tensor(n_before)[:, None] + ar(1, NFc + 1)[None, :]).to(torch.float32).to(dev)
                m, ys = self._msum, []
                for f in range(NFc):  # (in frame order, in float32: what keeps the mean independent of the chunking)
                    m = torch.where(mask[:, f, None], m + x[:, f], m)
                    ys.append(x[:, f] - (m / ntab[:, f, None] + 1e-8))
                y = torch.stack(ys, dim=1)
                self._msum = torch.where(fin[:, None].to(dev), torch.zeros((), device=dev), m)
            else:
                y = x
        else:
            y = torch.zeros(S, 0, M, device=dev)
        vbuf = torch.cat([self._held, y], dim=1)                                         # [S, G + NFc, M]
        top = G + NFc - 1
        v_of = lambda p: torch.where(p < h, p, G + p - h).clamp(max=top)  # noqa: E731  frame p of held ++ new, in vbuf
        count = torch.tensor([p[5] for p in plan])[:, None]
        take = lambda idx: vbuf.gather(1, idx.to(dev)[:, :, None].expand(-1, -1, M))  # noqa: E731
        if R > 0:
            rows = take(v_of(ar(R * stack)[None, :].expand(S, -1))).reshape(S, R, stack * M)
            rows = torch.where((ar(R)[None, :] < count).to(dev)[:, :, None], rows, torch.zeros((), device=dev))
        else:
            rows = torch.zeros(S, 0, stack * M, device=dev)
        i = ar(G)[None, :].expand(S, -1)
        self._held = take(torch.where(live, v_of(count * stack + i), i))
        src0 = nf[:, None] * step  # (a final feed keeps nothing: its carry is never read again)
        i = ar(L)[None, :].expand(S, -1)
        self._carry = buf.gather(1, torch.where(live, a_of(src0 + i), i).to(dev))
        return rows


def running_mean_log_mel(audio_arr: torch.Tensor, sample_rate: int, n_mel_bins: int = 80, frame_length: float = 0.025,
                         frame_step: float = 0.01, hertz_low: float = 125.0, hertz_high: float = 7600.0,
                         norm: str = "running") -> torch.Tensor:
    """The features StreamingFrontEnd(norm="running") gives a whole utterance, [frames, n_mel_bins], on the audio's device:
    log(mel + 1e-6) minus the per-bin mean of the frames so far (+1e-8) -- what a model that is to be streamed through the
    running-mean front end should be trained on in place of compute_mel_spectrograms.  It is one final feed of a 1-slot front end."""
    from types import SimpleNamespace

    hp = SimpleNamespace(mel_bins=n_mel_bins, frame_length=frame_length, frame_step=frame_step, hertz_low=hertz_low,
                         hertz_high=hertz_high, downsample_factor=1)
    n = int(audio_arr.shape[-1])
    fe = StreamingFrontEnd(hp, sample_rate, 1, max(1, n), 1, norm, device=audio_arr.device)
    fe.start([0])
    rows, _ = fe.feed(audio_arr.reshape(1, n), [n], [True])
    return rows[0]


# ---- text side ------------------------------------------------------------------------------------------------
def init_vocab() -> List[str]:
    """utils/vocabulary.py:3-8: index 0 is the blank ('')."""
    return ["", " ", "<s>", "</s>"] + list("abcdefghijklmnopqrstuvwxyz'")


def normalize_text(text: str) -> str:
    """utils/preprocessing.py:23-28."""
    return text.lower().replace('"', "")


class CharEncoder:
    """Character-level encoder over init_vocab() (utils/encoding.py:44-48 tf_vocab_encode = bytes_split + table lookup;
    the reference builds that table with default_value=0, utils/encoding.py:66-67: every byte outside the vocabulary
    -- digits, punctuation, each byte of a non-ASCII character -- becomes id 0, the blank)."""

    def __init__(self, vocab: Sequence[str] = None):
        self.vocab = list(vocab) if vocab is not None else init_vocab()
        self.index = {c: i for i, c in enumerate(self.vocab)}

    @property
    def vocab_size(self) -> int:
        return len(self.vocab)

    def encode(self, text: str) -> List[int]:
        # bytes_split: one token per UTF-8 byte (a non-ASCII character yields several unknown bytes -> several zeros)
        return [self.index.get(chr(b), 0) if b < 128 else 0 for b in text.encode("utf8")]

    def decode(self, ids) -> str:
        return "".join(self.vocab[int(i)] for i in ids if 0 <= int(i) < len(self.vocab))


def preprocess_text(text: str, encoder) -> Tuple[List[int], List[int]]:
    """utils/preprocessing.py:177-183: (labels, pred_inp = [0] ++ labels)."""
    enc = encoder.encode(normalize_text(text))
    return enc, [0] + enc


def make_record(audio: torch.Tensor, sample_rate: int, text: str, hp, encoder):
    """The 5 tensors of one training example (utils/preprocessing.py:283-289):
    (mel_specs f32 [T, mel_bins*downsample], pred_inp i32 [L+1], spec_length, label_length, labels i32 [L])."""
    mel = preprocess_audio(audio, sample_rate, hp)
    labels, pred_inp = preprocess_text(text, encoder)
    return (mel, torch.tensor(pred_inp, dtype=torch.int32), int(mel.shape[0]), len(labels),
            torch.tensor(labels, dtype=torch.int32))


def padded_batch(records):
    """dataset.padded_batch(batch_size, padded_shapes=([-1,-1],[-1],[],[],[-1])) (run_rnnt.py:78-83): zero padding to
    the longest example of the batch."""
    B = len(records)
    T = max(r[0].shape[0] for r in records)
    F = records[0][0].shape[1]
    U = max(r[1].shape[0] for r in records)
    L = max(max(r[4].shape[0] for r in records), 1)
    mel = torch.zeros(B, T, F)
    pred_inp = torch.zeros(B, U, dtype=torch.int32)
    labels = torch.zeros(B, L, dtype=torch.int32)
    for i, (m, pi, _, _, lab) in enumerate(records):
        mel[i, : m.shape[0]] = m
        pred_inp[i, : pi.shape[0]] = pi
        labels[i, : lab.shape[0]] = lab
    spec_lengths = torch.tensor([r[2] for r in records], dtype=torch.int32)
    label_lengths = torch.tensor([r[3] for r in records], dtype=torch.int32)
    return mel, pred_inp, spec_lengths, label_lengths, labels
