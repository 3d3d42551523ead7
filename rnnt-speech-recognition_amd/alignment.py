"""Forced alignment: the maximum-probability monotone path through the transducer lattice and the frame at which every label
is emitted (include/rnnt.h "Forced alignment"; csrc/align_kernels.hip).

  rnnt_align(acts, labels, input_lengths, label_lengths, blank_label=0, topology="standard") -> (token_frames, token_logp, scores)
  align_joint(joint, enc, pred, labels, input_lengths, label_lengths, slab_frames=None, topology="standard")
                                                 the same from enc / pred, in slabs
  token_times(token_frames, hp, sample_rate)     lattice frames -> seconds
  word_times(ids, token_frames, encoder)         character tokens -> (word, first_frame, last_frame)

Device tensors go through libwarprnnt.so.  CPU tensors run the SAME equations in torch (float32 log-softmax, float64 sweep, the
strict-greater tie rule): the mirror every module here has, so the host logic and its tests run without a GPU.  The two routes
agree wherever the best path's decisions are not within rounding of a tie (the normalisers differ in their last bits).

topology="standard" is the lattice of compute_rnnt_loss (a label edge stays on its frame; several labels may share a frame).
topology="modified" is the lattice of rnnt_loss(..., topology="modified") and of every decoder here: each frame emits exactly one
of {blank, next label}, token_frames is strictly increasing, scores <= -cost of the modified loss
(include/rnnt_modified_align.h; csrc/rnnt_modalign_kernels.hip in libwarprnnt_modalign.so)."""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import _lib

# align_joint: the logits of one slab of frames, [B, slab, U, V] float32, stay under this many bytes unless the caller says otherwise
SLAB_BYTES = 256 << 20
TOPOLOGIES = ("standard", "modified")


def _check_topology(topology, what):
    if topology not in TOPOLOGIES:
        raise ValueError(f"{what}: topology must be one of {TOPOLOGIES}, got {topology!r}")


def _as_i32(x, device) -> torch.Tensor:
    return torch.as_tensor(x).to(device=device, dtype=torch.int32).contiguous()


def _check(acts_shape, labels, input_lengths, label_lengths, what):
    B, T, U, V = acts_shape
    if V < 2:
        raise ValueError(f"{what}: the vocabulary needs at least two symbols")
    if U > 1 and tuple(labels.shape) != (B, U - 1):
        raise ValueError(f"{what}: labels must be [B, U-1] = [{B}, {U - 1}], got {tuple(labels.shape)}")
    if input_lengths.numel() != B or label_lengths.numel() != B:
        raise ValueError(f"{what}: input_lengths and label_lengths must be [B]")


# ---- the torch mirror -------------------------------------------------------------------------------------------------
def _torch_cells(acts, labels, blank):
    """{lpb, lpl} [B, T, U] float32 from float32 logits (labels clamped into the vocabulary, as the kernels do)."""
    B, T, U, V = acts.shape
    lp = torch.log_softmax(acts.float(), dim=-1)
    lpb = lp[..., blank]
    lpl = torch.zeros_like(lpb)
    if U > 1:
        idx = labels.long().clamp(0, V - 1)[:, None, :, None].expand(B, T, U - 1, 1)
        lpl[:, :, : U - 1] = lp[:, :, : U - 1].gather(3, idx)[..., 0]
    return lpb, lpl


def _torch_path(lpb, lpl, input_lengths, label_lengths):
    """The recurrence and the back-trace of include/rnnt.h on [B, T, U] cell log-probabilities: float64 values, anti-diagonal
    order, label arrival only if strictly greater."""
    B, T, U = lpb.shape
    dev = lpb.device
    il, ll = input_lengths.long(), label_lengths.long()
    bad = (il < 1) | (il > T) | (ll < 0) | (ll > U - 1)
    Tb, Ub = il.clamp(1, T), ll.clamp(0, U - 1)
    NEG = float("-inf")
    lpb64, lpl64 = lpb.double(), lpl.double()
    u = torch.arange(U, device=dev)
    N = T + U - 1
    v = torch.full((B, U), NEG, dtype=torch.float64, device=dev)
    v[:, 0] = 0.0
    took_label = torch.zeros(B, N, U, dtype=torch.bool, device=dev)
    final = torch.full((B,), NEG, dtype=torch.float64, device=dev)
    last = Tb - 1 + Ub
    rows = torch.arange(B, device=dev)
    final = torch.where(last == 0, v[rows, Ub], final)
    for n in range(1, N):
        ts = (n - 1 - u)  # frame of the source cells, diagonal n - 1
        src_ok = (ts[None, :] >= 0) & (ts[None, :] < Tb[:, None]) & (u[None, :] <= Ub[:, None])
        tsc = ts.clamp(0, T - 1)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        a = v + torch.where(src_ok, lpb64[:, tsc, u], zero)
        c = v + torch.where(src_ok, lpl64[:, tsc, u], zero)
        frm = torch.cat([torch.full((B, 1), NEG, dtype=torch.float64, device=dev), c[:, :-1]], dim=1)
        td = n - u
        dst_ok = (td[None, :] >= 0) & (td[None, :] < Tb[:, None]) & (u[None, :] <= Ub[:, None])
        lab = frm > a
        v = torch.where(dst_ok, torch.where(lab, frm, a), torch.full_like(a, NEG))
        took_label[:, n] = lab & dst_ok
        final = torch.where(last == n, v[rows, Ub], final)
    scores = final + lpb64[rows, Tb - 1, Ub]
    frames = torch.full((B, max(U - 1, 0)), -1, dtype=torch.int32)
    logp = torch.zeros(B, max(U - 1, 0), dtype=torch.float32)
    tl = took_label.cpu().numpy()
    lpl_c = lpl.cpu()
    for b in range(B):
        if bool(bad[b]):
            continue
        uu, n = int(Ub[b]), int(last[b])
        while n >= 1:
            if tl[b, n, uu]:
                frames[b, uu - 1] = n - uu
                logp[b, uu - 1] = lpl_c[b, n - uu, uu - 1]
                uu -= 1
            n -= 1
    scores = torch.where(bad, torch.full_like(scores, float("nan")), scores).float()
    return frames.to(dev), logp.to(dev), scores


def _torch_path_modified(lpb, lpl, input_lengths, label_lengths):
    """The recurrence and the back-trace of include/rnnt_modified_align.h on [B, T, U] cell log-probabilities: float64 values, row
    by row (every edge advances the frame), label arrival only if strictly greater, nodes outside the band u <= t,
    L - u <= T - t at -inf."""
    B, T, U = lpb.shape
    dev = lpb.device
    il, ll = input_lengths.long(), label_lengths.long()
    bad = (il < 1) | (il > T) | (ll < 0) | (ll > U - 1)
    Tb, Ub = il.clamp(1, T)[:, None], ll.clamp(0, U - 1)[:, None]
    lpb64, lpl64 = lpb.double(), lpl.double()
    u = torch.arange(U, device=dev)[None, :]
    neg = torch.full((B, U), float("-inf"), dtype=torch.float64, device=dev)
    v = neg.clone()
    v[:, 0] = 0.0
    took_label = torch.zeros(B, T + 1, U, dtype=torch.bool, device=dev)
    final = neg[:, 0].clone()

    def in_band(t):
        return (u <= t) & (u <= Ub) & (Ub - u <= Tb - t)

    for t in range(T):
        src_ok = in_band(t)
        stay = torch.where(src_ok, v + lpb64[:, t], neg)
        move = torch.where(src_ok & (u < Ub), v + lpl64[:, t], neg)
        frm = torch.cat([neg[:, :1], move[:, :-1]], dim=1)
        dst_ok = in_band(t + 1)
        lab = frm > stay
        v = torch.where(dst_ok, torch.where(lab, frm, stay), neg)
        took_label[:, t + 1] = lab & dst_ok
        final = torch.where(Tb[:, 0] == t + 1, v.gather(1, Ub)[:, 0], final)
    frames = torch.full((B, max(U - 1, 0)), -1, dtype=torch.int32)
    logp = torch.zeros(B, max(U - 1, 0), dtype=torch.float32)
    tl = took_label.cpu().numpy()
    lpl_c = lpl.cpu()
    for b in range(B):
        uu, t = int(Ub[b]), int(Tb[b])
        if bool(bad[b]) or uu > t:  # out-of-range lengths, or more labels than frames: no path
            continue
        while t >= 1:
            if tl[b, t, uu]:
                frames[b, uu - 1] = t - 1
                logp[b, uu - 1] = lpl_c[b, t - 1, uu - 1]
                uu -= 1
            t -= 1
    scores = torch.where(bad, torch.full_like(final, float("nan")), final).float()
    return frames.to(dev), logp.to(dev), scores


# ---- the engine ---------------------------------------------------------------------------------------------------
# per lattice: what the slab check calls it, the library, the workspace query and the stem of its three entry points
# (stem + "_cells", stem + "_path", stem: the whole tensor in one call)
_ENGINES = {
    "standard": ("align", _lib.load, _lib.align_workspace_bytes, "compute_rnnt_align"),
    "modified": ("align", _lib.load_modalign, _lib.modified_align_workspace_bytes, "compute_rnnt_modified_align"),
    "tdt": ("tdt align", _lib.load_tdtalign, _lib.tdt_align_workspace_bytes, "compute_rnnt_tdt_align"),
}


class _Aligner:
    """One alignment in flight on the engine: the workspace, the outputs and the slab feed.  A lattice whose entry points take
    more than the standard one's (tdt._TDTAligner) sets cell_args (after alphabet_size), path_args (after input_lengths),
    int_outputs and passes its logits' width and the extra arguments of its workspace query."""
    cell_args = path_args = ()
    int_outputs = 1  # int32 [B, U-1] outputs in front of token_logp

    def __init__(self, B, T, U, V, labels, input_lengths, label_lengths, blank, dev, topology="standard", width=None, ws_args=()):
        self.what, load, ws_bytes, self.stem = _ENGINES[topology]
        self.lib = load()
        self.B, self.T, self.U, self.V, self.blank, self.dev = B, T, U, V, int(blank), dev
        self.width = V if width is None else width
        self.labels = _as_i32(labels, dev)
        if self.labels.numel() == 0:
            self.labels = torch.zeros((B, 1), dtype=torch.int32, device=dev)
        self.il, self.ll = _as_i32(input_lengths, dev), _as_i32(label_lengths, dev)
        with torch.cuda.device(dev):
            self.ws = torch.empty(ws_bytes(T, U, B, *ws_args), dtype=torch.uint8, device=dev)

    def _opts(self):
        return _lib.make_options(torch.cuda.current_stream().cuda_stream, self.blank, self.T, self.U)

    def _run(self, suffix, *args):
        with torch.cuda.device(self.dev):
            st = getattr(self.lib, self.stem + suffix)(*args, self.ws.data_ptr(), self._opts())
        _lib.check(st, self.stem + suffix)

    def _outputs(self):
        n = max(self.U - 1, 1)
        out = [torch.empty(self.B, n, dtype=torch.int32, device=self.dev) for _ in range(self.int_outputs)]
        return out + [torch.empty(self.B, n, dtype=torch.float32, device=self.dev), torch.empty(self.B, dtype=torch.float32, device=self.dev)]

    def _trim(self, out):
        return tuple(x[:, : self.U - 1] for x in out[:-1]) + (out[-1],)

    def cells(self, slab: torch.Tensor, frame_offset: int) -> None:
        if slab.dtype != torch.float32 or slab.dim() != 4 or slab.shape[0] != self.B or tuple(slab.shape[2:]) != (self.U, self.width):
            raise ValueError(f"{self.what}: a slab must be float32 [{self.B}, frames, {self.U}, {self.width}], got {tuple(slab.shape)}")
        slab = slab.contiguous()
        self._run("_cells", slab.data_ptr(), slab.shape[1], int(frame_offset), self.labels.data_ptr(), self.ll.data_ptr(),
                  self.il.data_ptr(), self.V, *self.cell_args, self.B)

    def path(self):
        out = self._outputs()
        self._run("_path", *(x.data_ptr() for x in out), self.ll.data_ptr(), self.il.data_ptr(), *self.path_args, self.B)
        return self._trim(out)

    def whole(self, acts):
        """cells on every frame of `acts` (contiguous), then path, in one call of the library."""
        out = self._outputs()
        self._run("", acts.data_ptr(), self.labels.data_ptr(), self.ll.data_ptr(), self.il.data_ptr(), self.V, *self.cell_args, self.B,
                  *(x.data_ptr() for x in out))
        return self._trim(out)

    def slabs(self, joint, enc, pred, S):
        """cells on the logits of `joint`, S frames at a time, then path."""
        for t0 in range(0, self.T, S):
            slab = joint.cell_logits(enc[:, t0:t0 + S].contiguous(), pred)
            self.cells(slab, t0)
            del slab  # back to the allocator before the next slab is asked for: one slab of logits is alive at a time
        return self.path()


@torch.no_grad()
def rnnt_align(acts, labels, input_lengths, label_lengths, blank_label: int = 0, topology: str = "standard"):
    """Best path through the lattice of `acts` (RAW LOGITS [B, T, U, V] float32, the loss op's convention).

    Returns (token_frames i32 [B, U-1], token_logp f32 [B, U-1], scores f32 [B]): the frame at which label u is emitted (-1 past
    the utterance's labels), its log-probability there (0 past them) and the path's log-probability.  An utterance whose lengths
    are out of range comes back with a NaN score and -1 frames.  topology="modified": the one-symbol-per-frame lattice (strictly
    increasing frames; an utterance with more labels than frames has no path: score -inf, -1 frames)."""
    _check_topology(topology, "rnnt_align")
    if acts.dim() != 4:
        raise ValueError("rnnt_align: acts must be [B, T, U, V]")
    if acts.dtype != torch.float32:
        raise TypeError("rnnt_align: acts must be float32")
    B, T, U, V = acts.shape
    dev = acts.device
    labels = _as_i32(labels, dev)
    input_lengths, label_lengths = _as_i32(input_lengths, dev), _as_i32(label_lengths, dev)
    _check(acts.shape, labels, input_lengths, label_lengths, "rnnt_align")
    if not 0 <= int(blank_label) < V:
        raise ValueError("rnnt_align: blank_label outside the vocabulary")
    if not acts.is_cuda:
        lpb, lpl = _torch_cells(acts.detach(), labels, int(blank_label))
        path = _torch_path_modified if topology == "modified" else _torch_path
        return path(lpb, lpl, input_lengths, label_lengths)
    al = _Aligner(B, T, U, V, labels, input_lengths, label_lengths, blank_label, dev, topology)
    return al.whole(acts.detach().contiguous())


def slab_frames_for(B: int, T: int, U: int, V: int, slab_bytes: int = SLAB_BYTES) -> int:
    """Frames per slab so that [B, slab, U, V] float32 logits stay under slab_bytes (at least one frame)."""
    return int(max(1, min(T, slab_bytes // max(1, 4 * B * U * V))))


@torch.no_grad()
def align_joint(joint, enc, pred, labels, input_lengths, label_lengths, slab_frames: Optional[int] = None,
                slab_bytes: int = SLAB_BYTES, topology: str = "standard"):
    """rnnt_align on the logits of `joint` (a JointLoss) for enc [B, T, H] / pred [B, U, H] without holding [B, T, U, V]: the
    logits come from joint.cell_logits one slab of frames at a time, each slab is reduced to two floats per lattice cell
    (compute_rnnt_align_cells), and the sweep runs once.  slab_frames=None picks the largest slab whose logits stay under
    `slab_bytes` (default SLAB_BYTES = 256 MiB).  The outputs are bitwise those of rnnt_align on joint.cell_logits(enc, pred), with
    the same `topology`."""
    _check_topology(topology, "align_joint")
    B, T, _ = enc.shape
    U = pred.shape[1]
    V = joint.W2.shape[1]
    dev = enc.device
    labels = _as_i32(labels, dev)
    input_lengths, label_lengths = _as_i32(input_lengths, dev), _as_i32(label_lengths, dev)
    _check((B, T, U, V), labels, input_lengths, label_lengths, "align_joint")
    S = slab_frames_for(B, T, U, V, slab_bytes) if slab_frames is None else int(slab_frames)
    if S < 1:
        raise ValueError("align_joint: slab_frames must be positive")
    if not enc.is_cuda:
        parts = [_torch_cells(joint.cell_logits(enc[:, t0:t0 + S], pred).float(), labels, joint.blank_label) for t0 in range(0, T, S)]
        lpb, lpl = torch.cat([p[0] for p in parts], dim=1), torch.cat([p[1] for p in parts], dim=1)
        path = _torch_path_modified if topology == "modified" else _torch_path
        return path(lpb, lpl, input_lengths, label_lengths)
    return _Aligner(B, T, U, V, labels, input_lengths, label_lengths, joint.blank_label, dev, topology).slabs(joint, enc, pred, S)


# ---- frames -> time, tokens -> words ----------------------------------------------------------------------------------
def frame_seconds(hp, sample_rate) -> float:
    """Seconds of audio per lattice frame: the front end's frame step (in whole samples, as features.compute_mel_spectrograms
    rounds it) x the frames stacked by downsample_spec x the encoder's TimeReduction factor."""
    sr = float(sample_rate)
    step = int(round(sr * hp.frame_step))
    reduction = int(hp.time_reduction_factor) if 0 <= int(hp.time_reduction_index) < int(hp.encoder_layers) else 1
    return step * int(hp.downsample_factor) * reduction / sr


def token_times(token_frames, hp, sample_rate) -> torch.Tensor:
    """Start, in seconds, of the frame that emits each token (float64, same shape); NaN where token_frames is -1."""
    f = torch.as_tensor(token_frames)
    t = f.to(torch.float64) * frame_seconds(hp, sample_rate)
    return torch.where(f < 0, torch.full_like(t, float("nan")), t)


def word_times(ids, token_frames, encoder) -> List[Tuple[str, int, int]]:
    """Character vocabulary (features.CharEncoder): the tokens between spaces as (word, first_frame, last_frame).  `ids` and
    `token_frames` are one utterance's labels and emission frames; entries with a frame of -1 (padding) end the utterance."""
    ids = [int(i) for i in torch.as_tensor(ids).flatten().tolist()]
    frames = [int(f) for f in torch.as_tensor(token_frames).flatten().tolist()]
    space = encoder.index.get(" ")
    words, cur, first, last = [], [], None, None
    for i, f in zip(ids, frames):
        if f < 0:
            break
        if i == space:
            if cur:
                words.append(("".join(cur), first, last))
            cur, first, last = [], None, None
            continue
        ch = encoder.vocab[i] if 0 <= i < len(encoder.vocab) else ""
        if not ch:
            continue
        cur.append(ch)
        first = f if first is None else first
        last = f
    if cur:
        words.append(("".join(cur), first, last))
    return words
