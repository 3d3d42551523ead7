"""The token-and-duration (TDT) transducer loss (include/rnnt_tdt.h compute_rnnt_loss_tdt, libwarprnnt_tdt.so) and greedy TDT
decoding: batched (TDTGreedyJoint / tdt_greedy_search_batch on include/rnnt_tdt_greedy.h, libwarprnnt_tdtgreedy.so), over live
streams fed chunk by chunk (TDTGreedyStreamJoint / StreamingTDTGreedyDecoder on include/rnnt_tdt_stream.h, libwarprnnt_tdtstream.so)
and as a host loop over one utterance (tdt_greedy_decode); batched beam search with n-best lists (TDTBeamJoint /
tdt_beam_search_batch on include/rnnt_tdt_beam.h, libwarprnnt_tdtbeam.so) and the same search over live streams (TDTBeamStreamJoint /
StreamingTDTBeamDecoder on include/rnnt_tdt_beam_stream.h, libwarprnnt_tdtbeamstream.so); and forced alignment on the same lattice (rnnt_align_tdt / tdt_align_joint
on include/rnnt_tdt_align.h, libwarprnnt_tdtalign.so): per label of a given transcript the frame that emits it and the frames it claims.

The joint of a TDT model emits V token logits and D duration logits per lattice cell: acts [B, T, U, V + D].  An edge of the lattice
consumes d frames, d from `durations`; tokens and durations have a log-softmax each; `sigma` (>= 0) is subtracted from every token
log-probability (the logit under-normalisation of the paper).  From node (t, u), for each duration d_i:
    blank edge to (t + d_i, u)      lp(t,u,blank) - sigma + ld(t,u,i)   iff d_i > 0 and (t + d_i < T, or t + d_i == T and u == L)
    label edge to (t + d_i, u + 1)  lp(t,u,y_u)  - sigma + ld(t,u,i)   iff u < L and t + d_i < T
cost = -ln of the total weight of the paths from (0, 0) to the terminal (T, L).  An utterance without a path (durations [0, 2] with an
odd T; [1, 2] with L >= T) costs +inf with zero gradients.

    costs = rnnt_loss_tdt(acts, labels, input_lengths, label_lengths, durations=[0, 1, 2, 3, 4])

Device tensors run the HIP library (no eager fallback: a missing library is an error).  CPU tensors run a float64 torch mirror of
the same contract that autograd differentiates, so the module is usable without a device; the mirror returns float64 costs."""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._lib import ptr
from . import alignment as _alignment
from . import decoding as _decoding
from . import joint as _joint
from .loss import _as_i32

MAX_DURATIONS = 8  # include/rnnt_tdt.h: 1 <= D <= 8
MAX_DURATION = 8   # and durations[D - 1] <= 8
MAX_U = 1024       # maxU of compute_rnnt_loss_tdt
_NEG_INF = float("-inf")


# ---- arguments ----------------------------------------------------------------------------------------------------------
def check_durations(durations) -> tuple:
    """The duration set as a tuple of ints; ValueError unless it is strictly increasing, begins with 0 or 1, holds some d > 0, has
    1 ... 8 entries and none above 8 (include/rnnt_tdt.h)."""
    try:
        d = tuple(int(x) for x in durations)
        same = all(float(x) == float(int(x)) for x in durations)
    except (TypeError, ValueError):
        raise ValueError(f"durations must be a sequence of integers, got {durations!r}") from None
    ok = same and 1 <= len(d) <= MAX_DURATIONS and d[0] in (0, 1) and all(b > a for a, b in zip(d, d[1:]))
    if not ok or not 0 < d[-1] <= MAX_DURATION:
        raise ValueError(f"durations must be strictly increasing, begin with 0 or 1, hold some d > 0, have 1 ... {MAX_DURATIONS} "
                         f"entries and none above {MAX_DURATION}, got {durations!r}")
    return d


def check_sigma(sigma) -> float:
    s = float(sigma)
    if not (s >= 0.0 and math.isfinite(s)):  # (NaN fails the comparison)
        raise ValueError(f"sigma must be finite and >= 0, got {sigma!r}")
    return s


def _inputs(what, acts, labels, input_lengths, label_lengths, durations, blank_label, sigma):
    """Checks and conversions: (labels [B, >= 1] int32, input_lengths, label_lengths, durations, blank, sigma)."""
    dur, sigma = check_durations(durations), check_sigma(sigma)
    if not isinstance(acts, torch.Tensor) or acts.dim() != 4:
        raise ValueError(f"{what}: acts must be [B, T, U, V + D]")
    if acts.dtype != torch.float32 and (acts.is_cuda or acts.dtype != torch.float64):
        raise TypeError(f"{what}: acts must be float32 (float64 as well on the CPU)")
    B, T, U, R = acts.shape
    V = R - len(dur)
    if T < 1 or V < 2:
        raise ValueError(f"{what}: at least one frame and two tokens beside the {len(dur)} durations, got T = {T}, V + D = {R}")
    if not 1 <= U <= MAX_U:
        raise ValueError(f"{what}: acts must have 1 ... {MAX_U} label positions, got {U}")
    if labels.dim() != 2 or labels.shape[0] != B or labels.shape[1] != U - 1 and (U, labels.shape[1]) != (1, 1):
        raise ValueError(f"{what}: labels must be [B, U - 1] = [{B}, {U - 1}], got {tuple(labels.shape)}")
    if input_lengths.numel() != B or label_lengths.numel() != B:
        raise ValueError(f"{what}: input_lengths and label_lengths must be [B]")
    blank = int(blank_label)
    if not 0 <= blank < V:
        raise ValueError(f"{what}: blank_label must be in [0, {V}), got {blank_label!r}")
    dev = acts.device
    labels = _as_i32(labels, dev)
    if labels.numel() == 0:
        labels = torch.zeros((B, 1), dtype=torch.int32, device=dev)
    return labels, _as_i32(input_lengths, dev).reshape(B), _as_i32(label_lengths, dev).reshape(B), dur, blank, sigma


# ---- the device route ---------------------------------------------------------------------------------------------------
def _tdt_call(acts, grads, labels, input_lengths, label_lengths, scale, costs, ws, dur, blank, sigma):
    """compute_rnnt_loss_tdt on the current stream (grads / scale / costs: tensors or None)."""
    B, T, U, R = acts.shape
    d = (ctypes.c_int * len(dur))(*dur)
    with torch.cuda.device(acts.device):
        opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, int(blank), T, U)
        st = _lib.load_tdt().compute_rnnt_loss_tdt(
            acts.data_ptr(), ptr(grads), labels.data_ptr(), label_lengths.data_ptr(), input_lengths.data_ptr(), ptr(scale),
            R - len(dur), d, len(dur), sigma, B, ptr(costs), ws.data_ptr(), opts)
    _lib.check(st, "compute_rnnt_loss_tdt")


def _device_buffers(acts, num_durations):
    B, T, U, _ = acts.shape
    with torch.cuda.device(acts.device):
        ws = torch.empty(_lib.tdt_workspace_bytes(T, U, B, num_durations), dtype=torch.uint8, device=acts.device)
        costs = torch.empty(B, dtype=torch.float32, device=acts.device)
    return ws, costs


class _TDTLossFunction(torch.autograd.Function):
    """A forward-only call in forward, a gradient-only call in backward with the upstream gradient as cost_scale."""

    @staticmethod
    def forward(ctx, acts, labels, input_lengths, label_lengths, dur, blank, sigma):
        acts = acts.detach()
        ws, costs = _device_buffers(acts, len(dur))
        _tdt_call(acts, None, labels, input_lengths, label_lengths, None, costs, ws, dur, blank, sigma)
        ctx.save_for_backward(acts, labels, input_lengths, label_lengths, ws)
        ctx.args = (dur, blank, sigma)
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        acts, labels, input_lengths, label_lengths, ws = ctx.saved_tensors
        scale = grad_costs.to(device=acts.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(acts.device):
            grads = torch.empty_like(acts)
        _tdt_call(acts, grads, labels, input_lengths, label_lengths, scale, None, ws, *ctx.args)
        return (grads,) + (None,) * 6


# ---- the float64 torch mirror -------------------------------------------------------------------------------------------
def _lse(terms):
    """logsumexp over dim 0 of float64 [K, ...]: -inf (and a zero gradient, never NaN) where every term is -inf."""
    m = terms.max(dim=0).values.detach()
    ms = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    s = torch.exp(terms - ms).sum(dim=0)
    none = s == 0
    return torch.where(none, torch.full_like(s, _NEG_INF), ms + torch.log(torch.where(none, torch.ones_like(s), s)))


def _mirror(acts, labels, input_lengths, label_lengths, dur, blank, sigma):
    """costs [B] float64, differentiable in `acts` by autograd; all utterances advance together, one skewed row n = t + u of the
    lattice per step.  Out-of-range lengths as the op reports them (clamped; NaN cost and NaN gradients on the clamped lattice)."""
    B, T, U, R = acts.shape
    D = len(dur)
    V = R - D
    dev = acts.device
    x = acts.to(torch.float64)
    il, ll = input_lengths.to(torch.int64), label_lengths.to(torch.int64)
    bad = (il < 1) | (il > T) | (ll < 0) | (ll > U - 1)
    Tb, Lb = il.clamp(1, T)[:, None, None], ll.clamp(0, U - 1)[:, None, None]
    t = torch.arange(T, device=dev)[None, :, None]
    u = torch.arange(U, device=dev)[None, None, :]
    live = (t < Tb) & (u <= Lb)
    x = torch.where(live[..., None], x, torch.zeros_like(x))  # padded cells are not read
    lp = torch.log_softmax(x[..., :V], dim=-1) - sigma
    ld = torch.log_softmax(x[..., V:], dim=-1)
    y = torch.zeros((B, U), dtype=torch.int64, device=dev)
    y[:, : labels.shape[1]] = labels.to(torch.int64).clamp(0, V - 1)[:, : U]
    lpb, lpl = lp[..., blank], lp.gather(3, y[:, None, :, None].expand(B, T, U, 1))[..., 0]
    # the edge weights at their SOURCE, -inf where the edge does not exist, on skewed rows: [2 D][B, N, U]
    N = T + U
    rows, cols = (t + u).expand(1, T, U)[0], u.expand(1, T, U)[0]
    ninf = torch.full((), _NEG_INF, dtype=torch.float64, device=dev)

    def skew(w, exists):
        out = torch.full((B, N, U), _NEG_INF, dtype=torch.float64, device=dev)
        out[:, rows, cols] = torch.where(exists, w, ninf)
        return out

    wb = [skew(lpb + ld[..., i], live & (d > 0) & ((t + d < Tb) | ((t + d == Tb) & (u == Lb)))) for i, d in enumerate(dur)]
    wl = [skew(lpl + ld[..., i], live & (u < Lb) & (t + d < Tb)) for i, d in enumerate(dur)]
    first = torch.full((B, U), _NEG_INF, dtype=torch.float64, device=dev)
    first[:, 0] = 0.0
    pad = torch.full((B, 1), _NEG_INF, dtype=torch.float64, device=dev)
    alpha = [first]
    for n in range(1, N):
        terms = []
        for i, d in enumerate(dur):
            if d > 0 and n - d >= 0:
                terms.append(alpha[n - d] + wb[i][:, n - d])
            if n - d - 1 >= 0:
                terms.append(torch.cat([pad, (alpha[n - d - 1] + wl[i][:, n - d - 1])[:, :-1]], dim=1))
        alpha.append(_lse(torch.stack(terms)))
    alpha = torch.stack(alpha, dim=1)  # [B, N, U]
    b = torch.arange(B, device=dev)
    lnP = alpha[b, (Tb + Lb)[:, 0, 0], Lb[:, 0, 0]]
    costs = -lnP
    # Out-of-range lengths, as the op reports them: a NaN cost and NaN gradients on the clamped lattice, for that utterance alone.
    # autograd gives that only if the cost DEPENDS on those logits, hence sum(live logits) x NaN (x 0 for the other utterances, so
    # that their gradients stay clean); a torch.where on the cost would leave finite gradients.  bad.any() is a host sync, paid to
    # keep the extra pass over the logits off every ordinary call.
    if bool(bad.any()):
        factor = torch.where(bad, torch.full_like(costs, float("nan")), torch.zeros_like(costs))  # NaN for that utterance alone
        costs = costs + torch.where(live, x.sum(-1), torch.zeros_like(lpb)).sum((1, 2)) * factor
    return costs


# ---- the public surface -------------------------------------------------------------------------------------------------
def rnnt_loss_tdt(acts, labels, input_lengths, label_lengths, durations, blank_label: int = 0, sigma: float = 0.0):
    """costs [B] of the TDT lattice, differentiable in `acts`.

    acts [B, T, U, V + D] float32 RAW LOGITS (V token logits, then D = len(durations) duration logits); labels [B, U - 1];
    input_lengths / label_lengths [B].  The forward is one forward-only call of compute_rnnt_loss_tdt, the backward one gradient-only
    call with the upstream gradient as cost_scale.  float32 on a device, float64 from the CPU mirror."""
    labels, il, ll, dur, blank, sigma = _inputs("rnnt_loss_tdt", acts, labels, input_lengths, label_lengths, durations, blank_label, sigma)
    if not acts.is_cuda:
        return _mirror(acts, labels, il, ll, dur, blank, sigma)
    return _TDTLossFunction.apply(acts if acts.is_contiguous() else acts.contiguous(), labels, il, ll, dur, blank, sigma)


def rnnt_loss_tdt_and_grad(acts, labels, input_lengths, label_lengths, durations, blank_label: int = 0, sigma: float = 0.0):
    """compute_rnnt_loss_tdt as one combined call: (costs [B], grads [B, T, U, V + D]) with the gradients of cost_b (unscaled).  The
    arguments of rnnt_loss_tdt; no autograd graph is kept.  CPU tensors: the float64 mirror (float64 results)."""
    labels, il, ll, dur, blank, sigma = _inputs("rnnt_loss_tdt_and_grad", acts, labels, input_lengths, label_lengths, durations,
                                                blank_label, sigma)
    a = acts.detach().contiguous()
    if not a.is_cuda:
        a = a.to(torch.float64).requires_grad_(True)
        costs = _mirror(a, labels, il, ll, dur, blank, sigma)
        fin = torch.isfinite(costs) | torch.isnan(costs)  # (+inf: no path -- nothing to differentiate, the gradients are zeros)
        (g,) = torch.autograd.grad(torch.where(fin, costs, torch.zeros_like(costs)).sum(), a)
        return costs.detach(), g
    ws, costs = _device_buffers(a, len(dur))
    with torch.cuda.device(a.device):
        grads = torch.empty_like(a)
    _tdt_call(a, grads, labels, il, ll, None, costs, ws, dur, blank, sigma)
    return costs, grads


class TDTLoss(torch.nn.Module):
    """nn.Module wrapper of rnnt_loss_tdt; reduction 'none' returns the per-utterance costs."""

    def __init__(self, durations, blank_label: int = 0, sigma: float = 0.0, reduction: str = "none"):
        super().__init__()
        self.durations = check_durations(durations)
        self.sigma = check_sigma(sigma)
        if reduction not in ("none", "sum", "mean"):
            raise ValueError(reduction)
        self.blank_label = blank_label
        self.reduction = reduction

    def forward(self, acts, labels, input_lengths, label_lengths):
        costs = rnnt_loss_tdt(acts, labels, input_lengths, label_lengths, self.durations, self.blank_label, self.sigma)
        if self.reduction == "sum":
            return costs.sum()
        if self.reduction == "mean":
            return costs.mean()
        return costs


# ---- greedy decoding ----------------------------------------------------------------------------------------------------
def tdt_greedy_decode(logits_fn, T: int, durations, blank_label: int = 0, max_symbols_per_frame: int = 10):
    """Greedy TDT decoding as a host loop: (tokens, frames), the emitted tokens and the frame each was emitted on.

    logits_fn(t, tokens) -> [V + D] logits of frame t after the tokens emitted so far (the joint of the caller's model).  The token is
    the argmax of the first V entries, the duration d the one at the argmax of the last D.  A non-blank token is appended.  A blank
    with d == 0 advances by one frame (it would not move otherwise), and so does the max_symbols_per_frame-th emission in a row on
    one frame with d == 0.  Then t += d, until t >= T (the last jump may pass T).

    One call of logits_fn and one host read per decision, one utterance at a time: tdt_greedy_search_batch is the same rule for a
    whole batch with the joint, both argmaxes and the state update in the library."""
    dur = check_durations(durations)
    if int(max_symbols_per_frame) < 1:
        raise ValueError(f"max_symbols_per_frame must be at least 1, got {max_symbols_per_frame!r}")
    tokens, frames = [], []
    t, on_frame = 0, 0
    while t < T:
        logits = torch.as_tensor(logits_fn(t, list(tokens))).reshape(-1)
        V = logits.numel() - len(dur)
        if V < 2 or not 0 <= int(blank_label) < V:
            raise ValueError(f"logits_fn must return V + D = V + {len(dur)} logits with the blank inside [0, V), got {logits.numel()}")
        k = int(torch.argmax(logits[:V]))
        d = dur[int(torch.argmax(logits[V:]))]
        if k != int(blank_label):
            tokens.append(k)
            frames.append(t)
            on_frame += 1
            if d == 0 and on_frame >= int(max_symbols_per_frame):
                d = 1
        elif d == 0:
            d = 1
        if d > 0:
            on_frame = 0
        t += d
    return tokens, frames


# ---- batched greedy decoding --------------------------------------------------------------------------------------------
CHECK_EVERY = 32  # decode steps between two reads of the all-done word (the only host reads of the loop)
LAST_STEPS = 0    # decode steps the last tdt_greedy_search_batch took (timing tools)
_WORKSPACES = {}  # (device, stream) -> the workspace of the last batched decode there


def _cell_logits(joint, e, pred, pred_proj):
    """One joint cell per row in torch: e [B, H] against pred [B, H], or against pred_proj [B, >= J] = pred @ W1 already."""
    W1, b1, W2, b2 = (x.detach() for x in (joint.W1, joint.b1, joint.W2, joint.b2))
    if pred_proj is None:
        z = (e + pred.to(e.dtype)) @ W1 + b1
    else:
        z = e @ W1 + b1 + pred_proj[:, : W1.shape[1]].to(e.dtype)
    return torch.tanh(z) @ W2 + b2


def _heads(joint, durations):
    """The two heads of a TDT joint's W2 [J, V + D] -> (durations, D, V); ValueError unless V >= 2 and the blank is a token."""
    dur = check_durations(durations)
    R, blank = joint.W2.shape[1], int(joint.blank_label)
    V = R - len(dur)
    if V < 2 or not 0 <= blank < V:
        raise ValueError(f"TDTGreedyJoint: W2 must have V + D = V + {len(dur)} columns with V >= 2 and the blank inside [0, V), "
                         f"got {R} columns and blank_label = {blank}")
    return dur, len(dur), V


class TDTGreedyJoint(_joint._GreedyEngineJoint):
    """The joint of the batched greedy TDT decoder (tdt_greedy_search_batch), with the interface of joint.GreedyJoint: one lattice
    cell per hypothesis and step, the argmax of the token head and of the duration head, the two log-softmaxes of the decision and
    the decoder state in one pass.

    joint: any object with W1 [H, J], b1 [J], W2 [J, V + D], b2 [V + D] and blank_label -- the first V columns of W2 are the token
    head, the last D = len(durations) the duration head.  A joint.JointLoss built with vocab_size = V + D qualifies, and its
    .logits feed rnnt_loss_tdt.

    Device tensors on shapes the library takes run the ENGINE (include/rnnt_tdt_greedy.h compute_rnnt_tdt_greedy_begin / _step):
    the object owns the workspace and the joint-unit padding of W1 / b1 / W2, as GreedyJoint does.  CPU tensors, and shapes the
    library refuses, run the same state machine in torch, vectorised over the batch.

    begin(enc [B, T, H], frame_lengths [B], max_symbols [B] or None, max_per_frame >= 1, max_hyp_len) allocates the outputs (`hyps`
    [B, max_hyp_len] zero-filled, `lengths`, `scores`, `emitted`, `all_done`); step(pred [B, H]) or step(pred_proj=[B, Jp]) advances
    every hypothesis by one decision and returns `emitted` (the token per row, or -1).  all_done[0]: 0 running, 1 finished, 2 paused
    on a full `hyps` buffer (grow_hyps() resumes them).  token_times=True: `frames` int32 [B, max_hyp_len] (-1 where no token is)
    and `logp` [B, max_hyp_len] (0 there): per token the frame of its decision and the token plus the duration log-probability."""

    def __init__(self, joint, durations, joint_dtype: str = "auto", token_times: bool = False):
        self.durations, self.D, V = _heads(joint, durations)
        super().__init__(joint, joint_dtype, token_times)
        self.V = V

    # ---- engine
    def begin(self, enc, frame_lengths, max_symbols, max_per_frame: int, max_hyp_len: int):
        if int(max_per_frame) < 1:
            raise ValueError(f"max_per_frame must be at least 1, got {max_per_frame!r}")
        ep = self._begin(enc, frame_lengths, max_symbols, max_per_frame, max_hyp_len)
        if ep is None:
            return
        B, T = self.B, self.T
        frames, ms = self._keep
        dur = (ctypes.c_int * self.D)(*self.durations)
        with torch.cuda.device(enc.device):
            nbytes = _lib.tdt_greedy_workspace_bytes(T, B, self.Jp, self.V, self.D, self.dtype)
            self._ws = _joint._workspace(self._ws, nbytes, enc.device)
            self._opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, self.blank, T, 1)
            st = _lib.load_tdtgreedy().compute_rnnt_tdt_greedy_begin(
                ep.data_ptr(), frames.data_ptr(), ptr(ms), self.W2.data_ptr(), self.b2.data_ptr(), self.Jp, self.V, dur, self.D, B,
                int(max_per_frame), self.dtype, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_tdt_greedy_begin")

    def step(self, pred=None, logit_stats=None, *, pred_proj=None):
        """pred [B, H]: the prediction network's output of every row -> emitted [B] (int32, -1 where nothing was emitted).
        pred_proj [B, Jp] instead of pred: that output already through W1 (joint.PredictionStep); the step skips its matmul."""
        if not self.engine:
            return self._torch_step(pred, pred_proj)
        pp = torch.matmul(pred.float(), self.W1).contiguous() if pred_proj is None else _joint._projected_operand(pred_proj, self.Jp)
        st = _lib.load_tdtgreedy().compute_rnnt_tdt_greedy_step(
            pp.data_ptr(), self.hyps.data_ptr(), ptr(self.frames), ptr(self.logp), self.hyps.shape[1], self.lengths.data_ptr(),
            self.scores.data_ptr(), self.emitted.data_ptr(), self.all_done.data_ptr(), ptr(logit_stats), self.Jp, self.V, self.D,
            self.B, self.dtype, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_tdt_greedy_step")
        return self.emitted

    # ---- torch composition: the same state machine (tdt_greedy_update_kernel)
    def _torch_begin(self, enc, frames, maxsym, max_per_frame):
        super()._torch_begin(enc, frames, maxsym, max_per_frame)
        self._dur = torch.tensor(self.durations, dtype=torch.long, device=enc.device)

    @staticmethod
    def _head(x):
        """argmax (lowest index on ties; -1 when no logit is above -inf: a NaN never wins), the logit there, logsumexp."""
        clean = torch.where(torch.isnan(x), torch.full_like(x, _NEG_INF), x)
        k = torch.argmax(clean, dim=-1)
        M = x.gather(1, k[:, None])[:, 0]
        none = ~(clean > _NEG_INF).any(dim=-1)
        lse = torch.logsumexp(x, dim=-1)
        lp = torch.where(none, torch.full_like(M, float("nan")), M - lse)
        return torch.where(none, torch.full_like(k, -1), k), lp

    def _torch_step(self, pred, pred_proj=None):
        B, T, N, V = self.B, self.T, self.hyps.shape[1], self.V
        ar = torch.arange(B, device=self._enc.device)
        live = ~self._done & (self._n < self._maxsym.clamp(max=N))
        e = self._enc[ar, self._t.clamp(0, T - 1)]
        logits = _cell_logits(self.joint, e, pred, pred_proj)
        k, lpt = self._head(logits[:, :V])
        i, lpd = self._head(logits[:, V:])
        lp = (lpt + lpd).to(self.scores.dtype)
        self.scores = torch.where(live, self.scores + lp, self.scores)
        d = torch.where(i >= 0, self._dur[i.clamp(min=0)], torch.ones_like(i))
        emit = live & (k >= 0) & (k != self.blank)
        pos = self._n.clamp(max=N - 1)[:, None]
        self.hyps.scatter_(1, pos, torch.where(emit, k.to(torch.int32), self.hyps.gather(1, pos)[:, 0])[:, None])
        if self.token_times:  # (the frame of this decision: before the cursor moves on)
            fr = self._t if self._frame_base is None else self._t + self._frame_base
            self.frames.scatter_(1, pos, torch.where(emit, fr.to(torch.int32), self.frames.gather(1, pos)[:, 0])[:, None])
            self.logp.scatter_(1, pos, torch.where(emit, lp.to(self.logp.dtype), self.logp.gather(1, pos)[:, 0])[:, None])
        self._n = self._n + emit.long()
        self._nf = torch.where(emit, self._nf + 1, self._nf)
        forced = (d == 0) & (~emit | (self._nf >= self._cap))  # a blank with d = 0, or the cap reached on this frame: one frame on
        d = torch.where(forced, torch.ones_like(d), d)
        self._nf = torch.where(live & (d > 0), torch.zeros_like(self._nf), self._nf)
        self._t = torch.where(live, self._t + d, self._t)
        self._done = self._done | (live & ((self._t >= self._Tb) | (self._n >= self._maxsym)))
        self.lengths.copy_(self._n.to(torch.int32))
        self.emitted.copy_(torch.where(emit, k, torch.full_like(k, -1)).to(torch.int32))
        running, paused = ~self._done & (self._n < N), ~self._done & (self._n >= N)
        self.all_done.copy_(torch.where(running.any(), 0, torch.where(paused.any(), 2, 1)).to(torch.int32).reshape(1))
        return self.emitted


@torch.no_grad()
def tdt_greedy_search_batch(prediction, joint, enc: torch.Tensor, frame_lengths: torch.Tensor, durations, max_length=None,
                            max_symbols_per_frame: int = 10, check_every: int = CHECK_EVERY, prediction_route: str = "torch",
                            token_times: bool = False):
    """Greedy TDT search over encoder outputs enc [B, T', H] with frame_lengths [B]: (hyps [B, N] int32 zero-padded, lengths [B],
    scores [B][, frames [B, N], logp [B, N]]).  The loop of decoding.greedy_search_batch: one TDTGreedyJoint step per decision of
    every utterance, one host read per `check_every` steps, grow_hyps when every running hypothesis has filled the buffer.

    prediction: the prediction network (model.PredictionNetwork: an embedding and LSTM blocks), advanced for the rows that emitted
    a token; prediction_route "engine" steps it in the library (joint.PredictionStep).  joint / durations: as for TDTGreedyJoint.
    max_length: None (no bound), an int or a tensor [B]: tokens per utterance at most.  max_symbols_per_frame >= 1."""
    global LAST_STEPS
    _decoding._check_prediction(prediction_route)
    jg = TDTGreedyJoint(joint, durations, token_times=token_times)
    out, LAST_STEPS = _decoding._greedy_search(jg, _WORKSPACES, prediction, enc, frame_lengths, max_length, int(max_symbols_per_frame),
                                               check_every, prediction_route)
    return out


# ---- batched beam search ------------------------------------------------------------------------------------------------
_BEAM_WORKSPACES = {}  # (device, stream[, "timed"]) -> the workspace of the last tdt_beam_search_batch there
LAST_ACTIVE_ROWS = None  # tdt_beam_search_batch(count_active=True): joint rows evaluated per utterance (timing tools)


class TDTBeamJoint(_joint._EngineJoint):
    """The joint of the batched TDT beam search (tdt_beam_search_batch), with the interface of joint.BeamJoint: per frame the joint
    of every ACTIVE hypothesis of every beam (cursor == frame; a waiting hypothesis costs nothing), the token top-`beam` x durations
    candidates, ranking, merging on (sequence, cursor) and the new beams in one pass.  The rule: include/rnnt_tdt_beam.h.

    joint / durations: as for TDTGreedyJoint.  Device tensors on shapes the library takes run the ENGINE
    (compute_rnnt_tdt_beam_begin / _step / _results, libwarprnnt_tdtbeam.so); the object owns the workspace and the joint-unit
    padding of W1 / b1 / W2.  CPU tensors, and shapes the library refuses, run the same rule in torch: float64 scores, the same key
    order (per-utterance bookkeeping on the host).

    begin(enc [B, T, H], frame_lengths [B]); step(pred [B beam, H]) or step(pred_proj=[B beam, Jp]) -> (parents, emitted) int32
    [B beam]; results() -> (hyps [B, beam, T] int32 zero-padded, lengths [B, beam] int32, scores [B, beam]), best first, and with
    token_times=True two more: frames and durations int32 [B, beam, T] (-1 padded), per token the frame that emitted it and the
    frames it claims.  cursors() -> int32 [B, beam], the next frame every hypothesis reads (-1: empty slot).  step takes the
    diagnostics keywords topk_logits / topk_symbols [B beam, beam], dur_logits [B beam, D], lse [B beam, 2]: written for the rows
    that were active."""

    def __init__(self, joint, durations, beam: int = 4, joint_dtype: str = "auto", token_times: bool = False):
        if not 1 <= int(beam) <= 16:
            raise ValueError("TDTBeamJoint: beam must be in 1 ... 16")
        self.K = int(beam)
        self.durations, self.D, V = _heads(joint, durations)
        super().__init__(joint, joint_dtype, token_times)
        self.V = V
        self._N = None  # (the stream: the tokens a hypothesis may hold)

    def _args(self):
        return self.Jp, self.V, self.D, self.B, self.K, self.dtype, int(self.token_times), self._ws.data_ptr(), self._opts

    def begin(self, enc, frame_lengths):
        B, T = enc.shape[0], enc.shape[1]
        dev = enc.device
        self.B, self.T = B, T
        R = B * self.K
        self.parents = torch.arange(R, dtype=torch.int32, device=dev)
        self.emitted = torch.full((R,), -1, dtype=torch.int32, device=dev)
        frames = frame_lengths.to(device=dev, dtype=torch.int32).contiguous()
        if not self.engine:
            return self._torch_begin(enc, frames)
        ep = (torch.matmul(enc.float(), self.W1) + self.b1).contiguous()
        self._keep = frames
        dur = (ctypes.c_int * self.D)(*self.durations)
        with torch.cuda.device(dev):
            nbytes = _lib.tdt_beam_workspace_bytes(T, B, self.K, self.Jp, self.V, self.D, self.dtype, self.token_times)
            self._ws = _joint._workspace(self._ws, nbytes, dev)
            self._opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, self.blank, T, 1)
            st = _lib.load_tdtbeam().compute_rnnt_tdt_beam_begin(ep.data_ptr(), frames.data_ptr(), self.W2.data_ptr(), self.b2.data_ptr(),
                                                                 self.Jp, self.V, dur, self.D, B, self.K, self.dtype,
                                                                 int(self.token_times), self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_tdt_beam_begin")

    def step(self, pred=None, topk_logits=None, topk_symbols=None, dur_logits=None, lse=None, *, pred_proj=None):
        """pred [B beam, H]: the prediction network's output of every slot -> (parents, emitted), int32 [B beam].
        pred_proj [B beam, Jp] instead of pred: that output already through W1 (joint.PredictionStep); the step skips its matmul."""
        if not self.engine:
            return self._torch_step(pred, pred_proj, topk_logits, topk_symbols, dur_logits, lse)
        pp = torch.matmul(pred.float(), self.W1).contiguous() if pred_proj is None else _joint._projected_operand(pred_proj, self.Jp)
        st = _lib.load_tdtbeam().compute_rnnt_tdt_beam_step(pp.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(),
                                                            ptr(topk_logits), ptr(topk_symbols), ptr(dur_logits), ptr(lse), *self._args())
        _lib.check(st, "compute_rnnt_tdt_beam_step")
        return self.parents, self.emitted

    def results(self):
        out = self._results()
        return out[:3] + out[4:] if self.token_times else out[:3]

    def cursors(self):
        """int32 [B, beam]: the next frame every hypothesis of the current beams reads (-1: empty slot)."""
        return self._results()[3]

    def _results(self):
        B, K, T = self.B, self.K, self.T
        if not self.engine:
            return self._torch_results()
        dev = self.parents.device
        hyps = torch.empty(B, K, T, dtype=torch.int32, device=dev)
        lengths = torch.empty(B, K, dtype=torch.int32, device=dev)
        scores = torch.empty(B, K, dtype=torch.float32, device=dev)
        cursors = torch.empty(B, K, dtype=torch.int32, device=dev)
        frames = torch.empty(B, K, T, dtype=torch.int32, device=dev) if self.token_times else None
        durs = torch.empty(B, K, T, dtype=torch.int32, device=dev) if self.token_times else None
        st = _lib.load_tdtbeam().compute_rnnt_tdt_beam_results(hyps.data_ptr(), lengths.data_ptr(), scores.data_ptr(), cursors.data_ptr(),
                                                               ptr(frames), ptr(durs), *self._args())
        _lib.check(st, "compute_rnnt_tdt_beam_results")
        return (hyps, lengths, scores, cursors, frames, durs)

    # ---- torch composition: the rule of include/rnnt_tdt_beam.h with its two shortcuts (token top-K, then pair top-K)
    def _torch_begin(self, enc, frames):
        self._enc = enc
        self._Tb = [int(x) for x in frames.clamp(0, enc.shape[1]).tolist()]
        self._t = 0
        self._beams = [[((), 0, 0.0, ())] for _ in range(self.B)]  # (tokens, cursor, float64 score, (frame, duration) pairs)
        self._sdtype = torch.promote_types(enc.dtype, torch.float32)

    def _torch_step(self, pred, pred_proj, topk_logits, topk_symbols, dur_logits, lse_out):
        B, K, V, D = self.B, self.K, self.V, self.D
        t = self._t
        self._t += 1
        parents, emitted = list(range(B * K)), [-1] * (B * K)
        active = [b * K + i for b in range(B) if t < self._Tb[b] for i, h in enumerate(self._beams[b]) if h[1] == t]
        rows = {}
        if active:
            idx = torch.tensor(active, device=self._enc.device)
            rows = self._torch_rows(active, idx, self._enc[:, min(t, self.T - 1)][idx // K], pred, pred_proj, topk_logits,
                                    topk_symbols, dur_logits, lse_out)
        for b in range(B):
            if t < self._Tb[b]:
                self._torch_rank(b, t, rows, parents, emitted)
        dev = self.parents.device
        self.parents = torch.tensor(parents, dtype=torch.int32, device=dev)
        self.emitted = torch.tensor(emitted, dtype=torch.int32, device=dev)
        return self.parents, self.emitted

    def _torch_rows(self, active, idx, e, pred, pred_proj, topk_logits, topk_symbols, dur_logits, lse_out):
        """The joint of the active rows `active` (idx: the same as a tensor; e [rows, H]: each row's encoder frame) -> per row its
        token top-K, duration logits, both logsumexps and the blank's logit; the diagnostics are written on the way."""
        K, V = self.K, self.V
        rows = {}
        lg = _cell_logits(self.joint, e, None if pred is None else pred[idx], None if pred_proj is None else pred_proj[idx])
        tok, dur = lg[:, :V], lg[:, V:]
        lt, ld = torch.logsumexp(tok.double(), -1).tolist(), torch.logsumexp(dur.double(), -1).tolist()
        clean = torch.where(torch.isnan(tok) | (tok == _NEG_INF), torch.full_like(tok, _NEG_INF), tok)
        top_l, top_v = torch.sort(clean, dim=-1, descending=True, stable=True)  # (logit descending, symbol ascending)
        top_l, top_v = top_l[:, :K], top_v[:, :K]
        top_v = torch.where(top_l > _NEG_INF, top_v, torch.full_like(top_v, -1))
        if K > V:
            top_l = torch.nn.functional.pad(top_l, (0, K - V), value=_NEG_INF)
            top_v = torch.nn.functional.pad(top_v, (0, K - V), value=-1)
        for out, val in ((topk_logits, top_l), (topk_symbols, top_v), (dur_logits, dur)):
            if out is not None:
                out[idx] = val.to(out.dtype)
        if lse_out is not None:
            lse_out[idx] = torch.tensor(list(zip(lt, ld)), dtype=lse_out.dtype, device=lse_out.device)
        bl = tok[:, self.blank].tolist()
        for n, r in enumerate(active):
            rows[r] = (top_l[n].tolist(), top_v[n].tolist(), dur[n].tolist(), lt[n], ld[n], bl[n])
        return rows

    def _torch_rank(self, b, t, rows, parents, emitted):
        K, blank = self.K, self.blank
        beam = self._beams[b]
        cands = []  # (score, i, v or -1 for a stay, j)
        for i, (y, c, s, tt) in enumerate(beam):
            if c != t:
                cands.append((s, i, -1, 0))
                continue
            top_l, top_v, dur, lt, ld, bl = rows[b * K + i]
            if self._N is not None and len(y) >= self._N:  # the stream: a full hypothesis offers its blank alone
                top_l, top_v = [bl], [blank]
            mine = []
            for l, v in zip(top_l, top_v):
                if v < 0:
                    continue
                for j, dl in enumerate(dur):
                    sc = s + ((float(l) - lt) + (float(dl) - ld))
                    if sc == sc and sc > -math.inf:
                        mine.append((sc, i, v, j))
            mine.sort(key=lambda x: (-x[0], x[2], x[3]))
            cands += mine[:K]
        cands.sort(key=lambda x: (-x[0], x[1], x[2], x[3]))
        taken = cands[:K]
        if not taken:  # the beam is carried over, one frame on
            self._beams[b] = [(y, t + 1, s, tt) for y, c, s, tt in beam]
            return
        merged = []  # [tokens, cursor, score, pairs, parent, emitted]
        for sc, i, v, j in taken:
            y, c, _, tt = beam[i]
            em = -1
            if v >= 0:
                d = self.durations[j] or 1
                c = t + d
                if v != blank:
                    y, tt, em = y + (v,), tt + ((t, d),), v
            hit = next((m for m in merged if m[0] == y and m[1] == c), None)
            if hit is None:
                merged.append([y, c, sc, tt, i, em])
            else:
                hi, lo = max(hit[2], sc), min(hit[2], sc)
                hit[2] = hi + math.log1p(math.exp(lo - hi))
        merged.sort(key=lambda m: -m[2])  # (stable)
        self._beams[b] = [tuple(m[:4]) for m in merged]
        for k, m in enumerate(merged):
            parents[b * K + k], emitted[b * K + k] = b * K + m[4], m[5]

    def _torch_results(self):
        B, K, T = self.B, self.K, (self.T if self._N is None else self._N)
        hyps = torch.zeros(B, K, T, dtype=torch.int32)
        lengths = torch.zeros(B, K, dtype=torch.int32)
        scores = torch.full((B, K), -math.inf, dtype=torch.float64)
        cursors = torch.full((B, K), -1, dtype=torch.int32)
        frames = torch.full((B, K, T), -1, dtype=torch.int32)
        durs = torch.full((B, K, T), -1, dtype=torch.int32)
        for b, beam in enumerate(self._beams):
            for k, (y, c, s, tt) in enumerate(beam):
                n = len(y)
                lengths[b, k], scores[b, k], cursors[b, k] = n, s, c
                if n:
                    hyps[b, k, :n] = torch.tensor(y, dtype=torch.int32)
                    frames[b, k, :n] = torch.tensor([f for f, _ in tt], dtype=torch.int32)
                    durs[b, k, :n] = torch.tensor([d for _, d in tt], dtype=torch.int32)
        dev = self.parents.device
        out = (hyps.to(dev), lengths.to(dev), scores.to(device=dev, dtype=self._sdtype), cursors.to(dev))
        return out + ((frames.to(dev), durs.to(dev)) if self.token_times else (None, None))


@torch.no_grad()
def tdt_beam_search_batch(prediction, joint, enc: torch.Tensor, frame_lengths: torch.Tensor, durations, beam: int = 4,
                          prediction_route: str = "torch", token_times: bool = False, count_active: bool = False):
    """TDT beam search (one symbol per frame, include/rnnt_tdt_beam.h) over encoder outputs enc [B, T', H] with frame_lengths [B]
    -> (hyps int32 [B, beam, T'] zero-padded, lengths int32 [B, beam], scores [B, beam][, frames, durations int32 [B, beam, T']]):
    every utterance's n-best, best first (empty slots: length 0, score -inf).  beam = 1 is tdt_greedy_search_batch with
    max_symbols_per_frame = 1.

    The loop of decoding.beam_search_batch: T' steps without reading the host; per step the prediction network runs on all B beam
    rows, its output and LSTM state are gathered by `parents`, and the rows that emitted a token advance.  prediction /
    prediction_route / joint / durations: as for tdt_greedy_search_batch.  count_active (timing tools): LAST_ACTIVE_ROWS becomes a
    device tensor [B] of the joint rows evaluated per utterance (one more small torch op per step, still no host read)."""
    global LAST_ACTIVE_ROWS
    _decoding._check_prediction(prediction_route)
    B, T = enc.shape[0], enc.shape[1]
    dev = enc.device
    jb = TDTBeamJoint(joint, durations, int(beam), token_times=bool(token_times))
    active = torch.zeros(B, dtype=torch.int64, device=dev) if count_active else None
    Tb = frame_lengths.to(dev).clamp(0, T) if count_active else None

    def count(t):
        active.add_(((jb.cursors() == t) & (t < Tb)[:, None]).sum(1))

    out = _decoding._beam_search(jb, _BEAM_WORKSPACES, prediction, enc, frame_lengths, prediction_route, count if count_active else None)
    LAST_ACTIVE_ROWS = active
    return out


# ---- streaming greedy decoding ------------------------------------------------------------------------------------------
class TDTGreedyStreamJoint(TDTGreedyJoint):
    """The joint of the streaming greedy TDT decoder (StreamingTDTGreedyDecoder): TDTGreedyJoint's step over `slots` streams whose
    encoder frames arrive chunk by chunk, as joint.GreedyStreamJoint is GreedyJoint's.

    Device tensors on shapes the library takes run the ENGINE (include/rnnt_tdt_stream.h compute_rnnt_tdt_greedy_stream_begin /
    _feed / _step): the object owns the workspace (reused by the next begin when it is large enough); W1 / b1 and every slot's frame
    base live in it.  Otherwise the same state machine runs in torch.  `frames` and `logp` are always kept.

    begin(slots, max_chunk_frames (encoder frames per feed), max_per_frame >= 1, max_hyp_len) leaves every slot finished;
    feed(enc [slots, Te, H], frames [slots], reset, final, max_symbols) hands every slot its chunk (device int32 vectors, lists or
    None); then step(pred_proj=...) until all_done[0] is 1 (2: grow_hyps(), then go on), as for TDTGreedyJoint.  What a duration
    jump reaches beyond the chunk a slot holds is carried into its next chunks; `frames` count from the slot's reset."""

    def __init__(self, joint, durations, joint_dtype: str = "auto"):
        super().__init__(joint, durations, joint_dtype, token_times=True)

    def begin(self, slots: int, max_chunk_frames: int, max_per_frame: int, max_hyp_len: int, device=None):
        if int(max_per_frame) < 1:
            raise ValueError(f"max_per_frame must be at least 1, got {max_per_frame!r}")
        dev = self._begin_stream(slots, max_chunk_frames, max_per_frame, max_hyp_len, device)
        if not self.engine:
            self._dur = torch.tensor(self.durations, dtype=torch.long, device=dev)
            return
        S, T = self.B, self.T
        dur = (ctypes.c_int * self.D)(*self.durations)
        with torch.cuda.device(dev):
            nbytes = _lib.tdt_greedy_stream_workspace_bytes(T, S, self.H, self.Jp, self.V, self.D, self.dtype)
            self._ws = _joint._workspace(self._ws, nbytes, dev)
            self._opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, self.blank, T, 1)
            st = _lib.load_tdtstream().compute_rnnt_tdt_greedy_stream_begin(
                self.W1.data_ptr(), self.b1.data_ptr(), self.W2.data_ptr(), self.b2.data_ptr(), self.H, self.Jp, self.V, dur, self.D,
                S, self.dtype, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_tdt_greedy_stream_begin")

    def feed(self, enc, frames, reset=None, final=None, max_symbols=None):
        """enc [slots, Te, H] (None or Te = 0: no frames), frames [slots] encoder frames per slot, reset / final [slots] or None,
        max_symbols [slots] or None (the budget of the streams reset here)."""
        S = self.B
        Te = 0 if enc is None else int(enc.shape[1])
        if Te > self.Tc:
            raise ValueError(f"a feed takes at most {self.Tc} encoder frames, got {Te}")
        if not self.engine:
            return self._torch_feed(enc, Te, frames, reset, final, max_symbols)
        dev = self.hyps.device
        if Te > 0:
            enc = _joint._aligned16(enc.to(device=dev, dtype=torch.float32))
            if tuple(enc.shape) != (S, Te, self.H):
                raise ValueError(f"enc must be [{S}, frames, {self.H}], got {tuple(enc.shape)}")
        cv = lambda x: None if x is None else _joint._device_i32(x, dev).reshape(S)  # noqa: E731
        fr, rs, fi, ms = cv(frames), cv(reset), cv(final), cv(max_symbols)
        self._feed_args = (enc, fr, rs, fi, ms)  # (alive until the launches have read them)
        st = _lib.load_tdtstream().compute_rnnt_tdt_greedy_stream_feed(
            ptr(enc) if Te > 0 else None, Te, fr.data_ptr(), ptr(rs), ptr(fi), ptr(ms), self._cap, self.lengths.data_ptr(),
            self.scores.data_ptr(), self.all_done.data_ptr(), self.H, self.Jp, self.V, self.D, S, self.dtype, self._ws.data_ptr(),
            self._opts)
        _lib.check(st, "compute_rnnt_tdt_greedy_stream_feed")

    def step(self, pred=None, logit_stats=None, *, pred_proj=None):
        if not self.engine:
            return self._torch_step(pred, pred_proj)
        pp = torch.matmul(pred.float(), self.W1).contiguous() if pred_proj is None else _joint._projected_operand(pred_proj, self.Jp)
        st = _lib.load_tdtstream().compute_rnnt_tdt_greedy_stream_step(
            pp.data_ptr(), self.hyps.data_ptr(), self.frames.data_ptr(), self.logp.data_ptr(), self.hyps.shape[1],
            self.lengths.data_ptr(), self.scores.data_ptr(), self.emitted.data_ptr(), self.all_done.data_ptr(),
            ptr(logit_stats), self.Jp, self.V, self.D, self.B, self.dtype, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_tdt_greedy_stream_step")
        return self.emitted

    def _torch_feed(self, enc, Te, frames, reset, final, max_symbols):
        """tdt_stream_feed_kernel's state machine: the rule of include/rnnt_tdt_stream.h in its order."""
        S = self.B
        dev = self.hyps.device
        vec = lambda x, d: torch.full((S,), d, dtype=torch.long, device=dev) if x is None else torch.as_tensor(x).to(dev).reshape(S).long()  # noqa: E731
        rs, fi = vec(reset, 0) != 0, vec(final, 0) != 0
        ms = vec(max_symbols, 2**31 - 1).clamp(min=0)
        zero = torch.zeros_like(self._t)
        self._frame_base = torch.where(rs, zero, self._frame_base + self._Tb)
        skip = torch.where(rs, zero, (self._t - self._Tb).clamp(min=0))  # what the last jump reached beyond the chunk
        self._n = torch.where(rs, zero, self._n)
        self.scores = torch.where(rs, torch.zeros_like(self.scores), self.scores)
        self._maxsym = torch.where(rs, ms, self._maxsym)
        self._fin = self._fin & ~rs
        finished = self._fin | (self._n >= self._maxsym)
        self._Tb = torch.where(finished, zero, vec(frames, 0).clamp(0, Te))
        self._t = torch.where(finished, zero, skip)
        self._fin = finished | fi  # (after this chunk: a carry beyond a final chunk is dropped)
        self._nf = zero.clone()
        self._done = finished | (self._t >= self._Tb)
        H = self.joint.W1.shape[0]
        self._enc = enc if Te > 0 else torch.zeros(S, 1, H, dtype=self.joint.W1.dtype, device=dev)
        self.T = max(Te, 1)
        self.lengths.copy_(self._n.to(torch.int32))
        self.all_done.fill_(0 if bool((~self._done).any()) else 1)


class StreamingTDTGreedyDecoder(_decoding.StreamingGreedyDecoder):
    """Greedy TDT decoding of up to `slots` live audio streams at once, fed chunk by chunk (include/rnnt_tdt_stream.h): a
    decoding._StreamingSlots with the contract of decoding.StreamingGreedyDecoder -- start(slots), feed(mel_chunk, frames, final) ->
    (ids, counts), hypotheses(), timed_hypotheses(); non-final feeds bring multiples of the encoder's reduction factor; a feed
    reads the host for the all-done word every `check_every` steps and once for N -- and the step rule of tdt_greedy_search_batch.
    Its constructor, feed loop, slot handling and results ARE StreamingGreedyDecoder's; only the joint differs (_make_joint): a
    TDTGreedyStreamJoint.

    durations: the duration set of the model.  joint: an object with W1, b1, W2 [J, V + D], b2 and blank_label (TDTGreedyJoint's
    `joint`); None: model.joint.  max_symbols_per_frame >= 1 (mandatory for TDT: with a duration 0 an uncapped decode need not end).

    A duration jump that reaches beyond the frames a slot has so far is carried into its next feeds, and token frames count from
    the slot's start, so a stream fed through any chunking, in any slot, beside any other traffic ends with the ids, frames,
    log-probabilities, length and score of the same stream fed in one call to a 1-slot decoder (bitwise on an MI355X), and with the
    ids and frames of tdt_greedy_search_batch of the stream alone.  A jump beyond a stream's final frame is dropped."""

    def __init__(self, model, durations, slots: int, max_chunk_frames: int, joint=None, max_length=None,
                 max_symbols_per_frame: int = 10, check_every: int = CHECK_EVERY):
        if int(max_symbols_per_frame) < 1:
            raise ValueError(f"max_symbols_per_frame must be at least 1, got {max_symbols_per_frame!r}")
        self.durations = check_durations(durations)
        self._joint = model.joint if joint is None else joint
        super().__init__(model, slots, max_chunk_frames, max_length=max_length, max_symbols_per_frame=int(max_symbols_per_frame),
                         check_every=check_every, token_times=True)

    def _make_joint(self, model):
        return TDTGreedyStreamJoint(self._joint, self.durations)


# ---- streaming beam search ----------------------------------------------------------------------------------------------
class TDTBeamStreamJoint(TDTBeamJoint):
    """The joint of the streaming TDT beam search (StreamingTDTBeamDecoder): TDTBeamJoint's step over `slots` streams whose encoder
    frames arrive chunk by chunk, each slot keeping its beam from one feed to the next, as joint.BeamStreamJoint is BeamJoint's.
    The rule: include/rnnt_tdt_beam_stream.h.

    Device tensors on shapes the library takes run the ENGINE (compute_rnnt_tdt_beam_stream_begin / _feed / _step / _results,
    libwarprnnt_tdtbeamstream.so): the object owns the workspace; W1 / b1, every slot's frame base and every hypothesis's cursor
    live in it.  CPU tensors, and shapes the library refuses (at construction or at begin), run the same rule in torch with float64
    scores: TDTBeamJoint's rank and merge code, the capacity rule and both stable lengths included.

    begin(slots, max_chunk_frames (encoder frames per feed), max_hyp_len (the tokens a stream's hypothesis may hold)) leaves every
    slot finished with an empty beam; feed(enc [slots, Te, H], frames [slots], reset, final) hands every slot its chunk (int
    vectors, lists or None); then step(pred_proj=...) once per encoder frame of the longest chunk (host data: nothing is polled),
    each followed by a prediction-network step -- after the last frame too.  What a hypothesis's duration jump reaches beyond the
    chunk its slot holds is carried into the slot's next chunks.  results() -> (hyps [slots, beam, max_hyp_len] zero-padded,
    lengths [slots, beam], scores [slots, beam], stable [slots], cursors [slots, beam]) at any time, and with token_times=True
    three more: frames, durations int32 [slots, beam, max_hyp_len] (-1 padded) and timed_stable [slots].  Cursors and frames count
    from the slot's reset; stable is the common token prefix of a slot's hypotheses, timed_stable the prefix on which they agree
    in frame and duration too."""

    MAX_ROWS, MAX_WIDTH = 1024, 4096  # slots * beam: the prediction network's rows; the encoder width

    def _args(self):
        return self.Jp, self.V, self.D, self.B, self.K, self.N, self.dtype, int(self.token_times), self._ws.data_ptr(), self._opts

    def begin(self, slots: int, max_chunk_frames: int, max_hyp_len: int, device=None):
        S, T, N, K = int(slots), int(max_chunk_frames), int(max_hyp_len), self.K
        if S < 1 or S * K > self.MAX_ROWS:
            raise ValueError(f"slots * beam must be in 1 ... {self.MAX_ROWS}, got {S} * {K}")
        if T < 1 or N < 1:
            raise ValueError("max_chunk_frames and max_hyp_len must be >= 1")
        dev = self.W2.device if self.engine else (device if device is not None else self.joint.W2.device)
        self.B, self.T, self.Tc, self.N, self._N = S, T, T, N, N
        self.parents = torch.arange(S * K, dtype=torch.int32, device=dev)
        self.emitted = torch.full((S * K,), -1, dtype=torch.int32, device=dev)
        if self.engine:
            self.H = int(self.W1.shape[0])
            words = (6 if self.token_times else 2) * S * K * N
            if self.H > self.MAX_WIDTH or words >= 2**31 or S * T * self.Jp >= 2**31:
                self.engine = False  # (what only the stream refuses: the torch route takes it)
        if not self.engine:
            self._sdtype = torch.promote_types(self.joint.W2.dtype, torch.float32)
            self._beams = [[] for _ in range(S)]
            self._base, self._ct, self._Tb, self._fin = [0] * S, [0] * S, [0] * S, [True] * S
            self._enc = None
            return
        dur = (ctypes.c_int * self.D)(*self.durations)
        with torch.cuda.device(dev):
            nbytes = _lib.tdt_beam_stream_workspace_bytes(T, S, K, N, self.H, self.Jp, self.V, self.D, self.dtype, self.token_times)
            self._ws = _joint._workspace(self._ws, nbytes, dev)
            self._opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, self.blank, T, 1)
            st = _lib.load_tdtbeamstream().compute_rnnt_tdt_beam_stream_begin(
                self.W1.data_ptr(), self.b1.data_ptr(), self.W2.data_ptr(), self.b2.data_ptr(), self.H, self.Jp, self.V, dur, self.D,
                S, K, N, self.dtype, int(self.token_times), self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_tdt_beam_stream_begin")

    def feed(self, enc, frames, reset=None, final=None):
        """enc [slots, Te, H] (None or Te = 0: no frames), frames [slots] encoder frames per slot, reset / final [slots] or None."""
        S = self.B
        Te = 0 if enc is None else int(enc.shape[1])
        if Te > self.Tc:
            raise ValueError(f"a feed takes at most {self.Tc} encoder frames, got {Te}")
        if not self.engine:
            return self._torch_feed(enc, Te, frames, reset, final)
        dev = self.parents.device
        if Te > 0:
            enc = _joint._aligned16(enc.to(device=dev, dtype=torch.float32))
            if tuple(enc.shape) != (S, Te, self.H):
                raise ValueError(f"enc must be [{S}, frames, {self.H}], got {tuple(enc.shape)}")
        cv = lambda x: None if x is None else _joint._device_i32(x, dev).reshape(S)  # noqa: E731
        fr, rs, fi = cv(frames), cv(reset), cv(final)
        self._feed_args = (enc, fr, rs, fi)  # (alive until the launches have read them)
        st = _lib.load_tdtbeamstream().compute_rnnt_tdt_beam_stream_feed(
            ptr(enc) if Te > 0 else None, Te, fr.data_ptr(), ptr(rs), ptr(fi), self.H, self.Jp, self.V, self.D, S, self.K, self.N,
            self.dtype, int(self.token_times), self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_tdt_beam_stream_feed")

    def step(self, pred=None, topk_logits=None, topk_symbols=None, dur_logits=None, lse=None, *, pred_proj=None):
        """One frame of every slot that has one left -> (parents, emitted), int32 [slots beam]; the other slots are frozen."""
        if not self.engine:
            return self._torch_step(pred, pred_proj, topk_logits, topk_symbols, dur_logits, lse)
        pp = torch.matmul(pred.float(), self.W1).contiguous() if pred_proj is None else _joint._projected_operand(pred_proj, self.Jp)
        st = _lib.load_tdtbeamstream().compute_rnnt_tdt_beam_stream_step(
            pp.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(), ptr(topk_logits), ptr(topk_symbols), ptr(dur_logits),
            ptr(lse), *self._args())
        _lib.check(st, "compute_rnnt_tdt_beam_stream_step")
        return self.parents, self.emitted

    def results(self):
        S, K, N = self.B, self.K, self.N
        if not self.engine:
            return self._torch_stream_results()
        dev = self.parents.device
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)  # noqa: E731
        hyps, lengths, cursors, stable = i32(S, K, N), i32(S, K), i32(S, K), i32(S)
        scores = torch.empty(S, K, dtype=torch.float32, device=dev)
        frames, durs, tstable = (i32(S, K, N), i32(S, K, N), i32(S)) if self.token_times else (None, None, None)
        st = _lib.load_tdtbeamstream().compute_rnnt_tdt_beam_stream_results(
            hyps.data_ptr(), lengths.data_ptr(), scores.data_ptr(), cursors.data_ptr(), stable.data_ptr(), ptr(frames), ptr(durs),
            ptr(tstable), *self._args())
        _lib.check(st, "compute_rnnt_tdt_beam_stream_results")
        out = (hyps, lengths, scores, stable, cursors)
        return out + (frames, durs, tstable) if self.token_times else out

    def cursors(self):
        return self.results()[4]

    # ---- torch composition: cursors and frames are kept from the slot's reset (frame base + chunk-local), which is the rule of
    # include/rnnt_tdt_beam_stream.h read from outside: nothing needs rebasing at a feed
    def _torch_feed(self, enc, Te, frames, reset, final):
        S = self.B
        vec = lambda x: [0] * S if x is None else [int(v) for v in torch.as_tensor(x).reshape(S).tolist()]  # noqa: E731
        fr, rs, fi = vec(frames), vec(reset), vec(final)
        for s in range(S):
            if rs[s]:
                self._beams[s], self._base[s], self._fin[s] = [((), 0, 0.0, ())], 0, False
            elif not self._fin[s]:
                self._base[s] += self._Tb[s]
            self._ct[s] = 0
            if self._fin[s]:
                self._Tb[s] = 0
            else:
                self._Tb[s] = min(max(fr[s], 0), Te)
                self._fin[s] = bool(fi[s])  # (after this chunk; a carry beyond it is dropped)
        self._enc = enc

    def _torch_step(self, pred, pred_proj, topk_logits, topk_symbols, dur_logits, lse_out):
        S, K = self.B, self.K
        parents, emitted = list(range(S * K)), [-1] * (S * K)
        live = [s for s in range(S) if self._ct[s] < self._Tb[s]]
        now = {s: self._base[s] + self._ct[s] for s in live}  # the frame since the slot's reset
        active = [s * K + i for s in live for i, h in enumerate(self._beams[s]) if h[1] == now[s]]
        rows = {}
        if active:
            idx = torch.tensor(active, device=self._enc.device)
            at = torch.tensor([self._ct[r // K] for r in active], device=self._enc.device)
            rows = self._torch_rows(active, idx, self._enc[idx // K, at], pred, pred_proj, topk_logits, topk_symbols, dur_logits,
                                    lse_out)
        for s in live:
            self._torch_rank(s, now[s], rows, parents, emitted)
            self._ct[s] += 1
        dev = self.parents.device
        self.parents = torch.tensor(parents, dtype=torch.int32, device=dev)
        self.emitted = torch.tensor(emitted, dtype=torch.int32, device=dev)
        return self.parents, self.emitted

    def _torch_stream_results(self):
        hyps, lengths, scores, cursors, frames, durs = self._torch_results()
        stable, tstable = [], []
        for beam in self._beams:
            n = m = min((len(h[0]) for h in beam), default=0)
            for p in range(n - 1, -1, -1):
                if any(h[0][p] != beam[0][0][p] for h in beam):
                    n = p
                if any(h[0][p] != beam[0][0][p] or h[3][p] != beam[0][3][p] for h in beam):
                    m = p
            stable.append(n)
            tstable.append(m)
        dev = self.parents.device
        out = (hyps, lengths, scores, torch.tensor(stable, dtype=torch.int32, device=dev), cursors)
        return out + (frames, durs, torch.tensor(tstable, dtype=torch.int32, device=dev)) if self.token_times else out


class StreamingTDTBeamDecoder(_decoding.StreamingBeamDecoder):
    """TDT beam search (one symbol per frame, include/rnnt_tdt_beam_stream.h) of up to `slots` live audio streams at once, fed chunk
    by chunk: the streaming counterpart of tdt_beam_search_batch.  Its constructor, slot handling, feed loop and results ARE
    decoding.StreamingBeamDecoder's -- start(slots), feed(mel_chunk, frames, final) -> (ids, lengths, stable), hypotheses(),
    nbest() --; only the joint differs (_make_joint): a TDTBeamStreamJoint.  context= and lm= are not taken.

    durations: the duration set of the model.  joint: an object with W1, b1, W2 [J, V + D], b2 and blank_label (TDTGreedyJoint's
    `joint`); None: model.joint.  max_length: the tokens a stream's hypothesis may hold (StreamingBeamDecoder's rule: a full
    hypothesis goes on through blanks alone).

    token_times=True: timed_nbest() -> (ids, lengths, scores, frames, durations), frames and durations int32 [slots, beam, N] (-1
    padded; per token the encoder frame since the slot's start that emitted it and the frames it claims) in place of
    StreamingBeamDecoder's log-probabilities, which the TDT beams do not keep; timed_hypotheses() -> the best (ids, frames,
    durations); timed_stable_lengths() -> the prefix of every slot on which its hypotheses agree in token, frame and duration.
    cursors() -> int32 [slots, beam]: the next frame since the slot's start every hypothesis reads.

    A hypothesis's duration jump beyond the frames its slot has so far is carried into the slot's next feeds, so a stream fed
    through any chunking, in any slot, beside any other traffic ends with the n-best (ids, lengths, scores, cursors, frames,
    durations) and both stable lengths of the same stream fed in one call to a 1-slot decoder: bitwise on an MI355X.  beam = 1
    gives the ids and frames of StreamingTDTGreedyDecoder with max_symbols_per_frame = 1."""

    def __init__(self, model, durations, slots: int, max_chunk_frames: int, beam: int = 4, joint=None, max_length=None,
                 token_times: bool = False):
        self.durations = check_durations(durations)
        self._joint = model.joint if joint is None else joint
        super().__init__(model, slots, max_chunk_frames, beam=beam, max_length=max_length, token_times=token_times)

    def _make_joint(self, model, K, context, lm):
        return TDTBeamStreamJoint(self._joint, self.durations, K, token_times=self.token_times)

    def cursors(self):
        return self.bj.results()[4]

    def bias_states(self):
        raise RuntimeError("the TDT beam search takes no context graph")

    def lm_states(self):
        raise RuntimeError("the TDT beam search takes no language model")

    def timed_hypotheses(self):
        """The best hypothesis of each slot with its times: (ids int32 [slots, N] zero-padded, frames, durations int32 [slots, N]
        -1 padded).  Needs token_times=True."""
        r = self._timed()
        return r[0][:, 0], r[5][:, 0], r[6][:, 0]

    def timed_nbest(self):
        """(ids [slots, beam, N], lengths [slots, beam], scores [slots, beam], frames [slots, beam, N], durations [slots, beam, N]),
        best first.  Needs token_times=True."""
        r = self._timed()
        return r[0], r[1], r[2], r[5], r[6]

    def timed_stable_lengths(self):
        """int32 [slots]: the leading tokens of a slot on which every hypothesis of its beam agrees in token, emission frame AND
        duration.  Never more than feed()'s `stable`.  Needs token_times=True."""
        return self._timed()[7]


# ---- forced alignment on the TDT lattice --------------------------------------------------------------------------------
def _align_cells_torch(acts, labels, dur, blank, sigma):
    """The float32 edge weights of include/rnnt_tdt_align.h from float32 logits, each operation rounded once: (wb, wl, raw), each
    [B, T, U, D]; raw = lp(label) + ld, the token_logp of a label edge (no sigma).  Labels are clamped into [0, V)."""
    x = acts.detach().to(torch.float32)
    B, T, U, R = x.shape
    V = R - len(dur)
    lp, ld = torch.log_softmax(x[..., :V], dim=-1), torch.log_softmax(x[..., V:], dim=-1)
    y = torch.zeros((B, U), dtype=torch.int64, device=x.device)
    y[:, : labels.shape[1]] = labels.to(torch.int64).clamp(0, V - 1)[:, :U]
    lpb, lpl = lp[..., blank], lp.gather(3, y[:, None, :, None].expand(B, T, U, 1))[..., 0]
    s = torch.tensor(sigma, dtype=torch.float32, device=x.device)
    return ((lpb - s)[..., None] + ld), ((lpl - s)[..., None] + ld), (lpl[..., None] + ld)


def _align_path_torch(wb, wl, raw, input_lengths, label_lengths, dur):
    """The recurrence, the tie rule and the back-trace of include/rnnt_tdt_align.h on float32 weights [B, T, U, D]: float64 values,
    one skewed row n = t + u per step with every utterance and column at once; per node the candidates in increasing i, the blank
    arrival before the label arrival, a candidate replacing the incumbent only if STRICTLY greater.  The weight of an edge that does
    not exist is selected away before it is added."""
    B, T, U, D = wb.shape
    dev = wb.device
    il, ll = input_lengths.to(torch.int64), label_lengths.to(torch.int64)
    bad = (il < 1) | (il > T) | (ll < 0) | (ll > U - 1)
    Tb, Lb = il.clamp(1, T)[:, None, None], ll.clamp(0, U - 1)[:, None, None]
    t = torch.arange(T, device=dev)[None, :, None]
    u = torch.arange(U, device=dev)[None, None, :]
    live = (t < Tb) & (u <= Lb)
    N = T + U
    rows, cols = (t + u).expand(1, T, U)[0], u.expand(1, T, U)[0]
    ninf = torch.full((), _NEG_INF, dtype=torch.float64, device=dev)

    def skew(w, exists):  # the weights at their SOURCE on skewed rows, -inf where the edge does not exist
        out = torch.full((B, N, U), _NEG_INF, dtype=torch.float64, device=dev)
        out[:, rows, cols] = torch.where(exists, w.to(torch.float64), ninf)
        return out

    wbs = [skew(wb[..., i], live & (d > 0) & ((t + d < Tb) | ((t + d == Tb) & (u == Lb)))) for i, d in enumerate(dur)]
    wls = [skew(wl[..., i], live & (u < Lb) & (t + d < Tb)) for i, d in enumerate(dur)]
    first = torch.full((B, U), _NEG_INF, dtype=torch.float64, device=dev)
    first[:, 0] = 0.0
    pad = torch.full((B, 1), _NEG_INF, dtype=torch.float64, device=dev)
    v = [first]
    codes = torch.full((B, N, U), -1, dtype=torch.int16, device=dev)
    for n in range(1, N):
        best = torch.full((B, U), _NEG_INF, dtype=torch.float64, device=dev)
        code = torch.full((B, U), -1, dtype=torch.int16, device=dev)
        for i, d in enumerate(dur):
            cands = []
            if d > 0 and n - d >= 0:
                cands.append((2 * i, v[n - d] + wbs[i][:, n - d]))
            if n - d - 1 >= 0:
                cands.append((2 * i + 1, torch.cat([pad, (v[n - d - 1] + wls[i][:, n - d - 1])[:, :-1]], dim=1)))
            for c, cand in cands:
                take = cand > best  # (a NaN never wins)
                best = torch.where(take, cand, best)
                code = torch.where(take, torch.full_like(code, c), code)
        v.append(best)
        codes[:, n] = code
    v = torch.stack(v, dim=1)  # [B, N, U]
    b = torch.arange(B, device=dev)
    Tn, Ln = Tb[:, 0, 0], Lb[:, 0, 0]
    scores = v[b, Tn + Ln, Ln]
    n_out = max(U - 1, 0)
    frames = torch.full((B, n_out), -1, dtype=torch.int32)
    durs = torch.full((B, n_out), -1, dtype=torch.int32)
    logp = torch.zeros(B, n_out, dtype=torch.float32)
    cd, raw_c = codes.cpu().numpy(), raw.cpu()
    for k in range(B):
        if bool(bad[k]) or not bool(scores[k] > _NEG_INF):
            continue
        uu, n = int(Ln[k]), int(Tn[k] + Ln[k])
        while n > 0:
            c = int(cd[k, n, uu])
            i, label = c >> 1, c & 1
            d = dur[i]
            if label:
                frames[k, uu - 1], durs[k, uu - 1] = n - uu - d, d
                logp[k, uu - 1] = raw_c[k, n - uu - d, uu - 1, i]
                uu -= 1
            n -= d + label
    scores = torch.where(bad, torch.full_like(scores, float("nan")), scores).float()
    return frames.to(dev), durs.to(dev), logp.to(dev), scores


class _TDTAligner(_alignment._Aligner):
    """One TDT alignment in flight on the engine (libwarprnnt_tdtalign.so): alignment._Aligner with the durations and sigma in its
    calls and token_durations among its outputs."""
    int_outputs = 2

    def __init__(self, B, T, U, V, labels, input_lengths, label_lengths, dur, blank, sigma, dev):
        d = (ctypes.c_int * len(dur))(*dur)
        self.cell_args, self.path_args = (d, len(dur), sigma), (d, len(dur))
        super().__init__(B, T, U, V, labels, input_lengths, label_lengths, blank, dev, "tdt", width=V + len(dur), ws_args=(len(dur),))


@torch.no_grad()
def rnnt_align_tdt(acts, labels, input_lengths, label_lengths, durations, blank_label: int = 0, sigma: float = 0.0):
    """Best path through the TDT lattice of `acts` (RAW LOGITS [B, T, U, V + D] float32, the convention of rnnt_loss_tdt):
    (token_frames i32 [B, U-1], token_durations i32 [B, U-1], token_logp f32 [B, U-1], scores f32 [B]) -- per label the frame that
    emits it and the frames it claims (-1 past the utterance's labels), the log-probability of the token and of its duration there,
    without sigma (0 past them), and the path's log-probability (sigma included; never above -rnnt_loss_tdt).  Frames are
    non-decreasing, equal only across duration 0.  An utterance without a path: score -inf, -1 and 0 elsewhere; out-of-range lengths:
    a NaN score for that utterance alone.  Device tensors run libwarprnnt_tdtalign.so (include/rnnt_tdt_align.h; a missing library
    is an error); CPU tensors run the same equations in torch: float32 log-softmaxes, float64 sweep, the same tie rule."""
    labels, il, ll, dur, blank, sigma = _inputs("rnnt_align_tdt", acts, labels, input_lengths, label_lengths, durations, blank_label,
                                                sigma)
    B, T, U, R = acts.shape
    if not acts.is_cuda:
        wb, wl, raw = _align_cells_torch(acts, labels, dur, blank, sigma)
        return _align_path_torch(wb, wl, raw, il, ll, dur)
    al = _TDTAligner(B, T, U, R - len(dur), labels, il, ll, dur, blank, sigma, acts.device)
    return al.whole(acts.detach().contiguous())


@torch.no_grad()
def tdt_align_joint(joint, enc, pred, labels, input_lengths, label_lengths, durations, slab_frames=None,
                    slab_bytes=_alignment.SLAB_BYTES, sigma: float = 0.0):
    """rnnt_align_tdt on the logits of `joint` for enc [B, T, H] / pred [B, U, H] without holding [B, T, U, V + D].  joint: any joint
    with V + D columns, cell_logits and blank_label -- a joint.JointLoss with vocab_size = V + D, as TDTGreedyJoint documents.  The
    logits come from joint.cell_logits one slab of frames at a time, each slab is reduced to 2 D floats per lattice cell
    (compute_rnnt_tdt_align_cells), one slab is alive at a time and the sweep runs once.  slab_frames=None picks the largest slab
    whose logits stay under slab_bytes (default alignment.SLAB_BYTES).  The outputs are bitwise those of rnnt_align_tdt on
    joint.cell_logits(enc, pred)."""
    dur, sigma = check_durations(durations), check_sigma(sigma)
    if enc.dim() != 3 or pred.dim() != 3 or enc.shape[0] != pred.shape[0]:
        raise ValueError("tdt_align_joint: enc must be [B, T, H] and pred [B, U, H]")
    B, T, _ = enc.shape
    U = pred.shape[1]
    R = int(joint.W2.shape[1])
    V = R - len(dur)
    blank = int(joint.blank_label)
    if T < 1 or V < 2 or not 0 <= blank < V:
        raise ValueError(f"tdt_align_joint: the joint must have V + D = V + {len(dur)} columns with V >= 2 and the blank inside "
                         f"[0, V), got {R} columns and blank_label = {blank}")
    if not 1 <= U <= MAX_U:
        raise ValueError(f"tdt_align_joint: pred must have 1 ... {MAX_U} label positions, got {U}")
    labels = torch.as_tensor(labels)
    if labels.dim() != 2 or labels.shape[0] != B or labels.shape[1] != U - 1 and (U, labels.shape[1]) != (1, 1):
        raise ValueError(f"tdt_align_joint: labels must be [B, U - 1] = [{B}, {U - 1}], got {tuple(labels.shape)}")
    dev = enc.device
    labels = _as_i32(labels, dev)
    if labels.numel() == 0:
        labels = torch.zeros((B, 1), dtype=torch.int32, device=dev)
    il, ll = _as_i32(input_lengths, dev).reshape(-1), _as_i32(label_lengths, dev).reshape(-1)
    if il.numel() != B or ll.numel() != B:
        raise ValueError("tdt_align_joint: input_lengths and label_lengths must be [B]")
    S = _alignment.slab_frames_for(B, T, U, R, int(slab_bytes)) if slab_frames is None else int(slab_frames)
    if S < 1:
        raise ValueError("tdt_align_joint: slab_frames must be positive")
    if not enc.is_cuda:
        parts = [_align_cells_torch(joint.cell_logits(enc[:, t0:t0 + S], pred), labels, dur, blank, sigma) for t0 in range(0, T, S)]
        wb, wl, raw = (torch.cat([p[k] for p in parts], dim=1) for k in range(3))
        return _align_path_torch(wb, wl, raw, il, ll, dur)
    return _TDTAligner(B, T, U, V, labels, il, ll, dur, blank, sigma, dev).slabs(joint, enc, pred, S)


def token_end_frames(token_frames, token_durations) -> torch.Tensor:
    """The first frame after the ones each token claims: token_frames + token_durations, -1 where token_frames is -1."""
    f, d = torch.as_tensor(token_frames), torch.as_tensor(token_durations)
    return torch.where(f < 0, torch.full_like(f, -1), f + d)
