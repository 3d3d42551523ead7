"""The CTC loss and the greedy CTC decoder of an auxiliary CTC head on the encoder (include/rnnt_ctc.h, libwarprnnt_ctc.so): the
second term of a hybrid objective, loss = transducer + w * ctc, with this library's conventions for the blank, the lengths and
infinite costs.

    costs = ctc_loss(logits, labels, input_lengths, label_lengths, blank_label=0)      # [B], autograd in logits
    costs, grads = ctc_loss_and_grad(logits, labels, input_lengths, label_lengths)     # one call, no graph
    tokens, lengths = ctc_greedy_decode(logits, input_lengths)                         # [B, T] padded with -1, [B]

logits [B, T, V] are raw (the log-softmax is fused), labels [B, L_max].  An utterance without a path (T_b < L_b + the number of
adjacent equal labels) costs +inf with zero gradients (`zero_infinity` turns the cost into 0); out-of-range lengths or a label
equal to the blank give NaN for that utterance alone.

Device tensors run the HIP library (no eager fallback: a missing library is an error).  CPU tensors run a float64 torch mirror of
the same rule, so the module is usable without a device; the mirror returns costs in the dtype of the logits."""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from ._lib import ptr
from .loss import _as_i32

_NEG_INF = float("-inf")
MAX_LABELS = 8191  # include/rnnt_ctc.h: maxU = L_max + 1 <= 8192


# ---- arguments ----------------------------------------------------------------------------------------------------------
def _check_logits(what, logits, blank_label):
    if not isinstance(logits, torch.Tensor) or logits.dim() != 3:
        raise ValueError(f"{what}: logits must be [B, T, V]")
    if logits.dtype != torch.float32 and (logits.is_cuda or logits.dtype != torch.float64):
        raise TypeError(f"{what}: logits must be float32 (float64 as well on the CPU)")
    B, T, V = logits.shape
    if B < 1 or T < 1 or V < 2:
        raise ValueError(f"{what}: at least one utterance, one frame and two symbols, got {tuple(logits.shape)}")
    blank = int(blank_label)
    if not 0 <= blank < V:
        raise ValueError(f"{what}: blank_label must be in [0, {V}), got {blank_label!r}")
    return blank


def _inputs(what, logits, labels, input_lengths, label_lengths, blank_label):
    """Checks and conversions: (labels [B, >= 1] int32, input_lengths, label_lengths, blank, maxU)."""
    blank = _check_logits(what, logits, blank_label)
    B = logits.shape[0]
    if labels.dim() != 2 or labels.shape[0] != B:
        raise ValueError(f"{what}: labels must be [B, L_max] = [{B}, L_max], got {tuple(labels.shape)}")
    if labels.shape[1] > MAX_LABELS:
        raise ValueError(f"{what}: at most {MAX_LABELS} labels per utterance, got {labels.shape[1]}")
    if input_lengths.numel() != B or label_lengths.numel() != B:
        raise ValueError(f"{what}: input_lengths and label_lengths must be [B]")
    dev = logits.device
    maxU = labels.shape[1] + 1
    labels = _as_i32(labels, dev)
    if labels.numel() == 0:
        labels = torch.zeros((B, 1), dtype=torch.int32, device=dev)  # (maxU = 1: a column nobody reads)
    return labels, _as_i32(input_lengths, dev).reshape(B), _as_i32(label_lengths, dev).reshape(B), blank, maxU


# ---- the device route ---------------------------------------------------------------------------------------------------
def _ctc_call(logits, grads, labels, input_lengths, label_lengths, scale, costs, ws, blank, maxU):
    """compute_rnnt_ctc_loss on the current stream (grads / scale / costs: tensors or None)."""
    B, T, V = logits.shape
    with torch.cuda.device(logits.device):
        opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, int(blank), T, maxU)
        st = _lib.load_ctc().compute_rnnt_ctc_loss(logits.data_ptr(), ptr(grads), labels.data_ptr(), label_lengths.data_ptr(),
                                                   input_lengths.data_ptr(), ptr(scale), V, B, ptr(costs), ws.data_ptr(), opts)
    _lib.check(st, "compute_rnnt_ctc_loss")


def _device_buffers(logits, maxU):
    B, T, _ = logits.shape
    with torch.cuda.device(logits.device):
        ws = torch.empty(_lib.ctc_workspace_bytes(T, maxU, B), dtype=torch.uint8, device=logits.device)
        costs = torch.empty(B, dtype=torch.float32, device=logits.device)
    return ws, costs


class _CTCLossFunction(torch.autograd.Function):
    """A forward-only call in forward, a gradient-only call in backward with the upstream gradient as cost_scale."""

    @staticmethod
    def forward(ctx, logits, labels, input_lengths, label_lengths, blank, maxU):
        logits = logits.detach().contiguous()
        ws, costs = _device_buffers(logits, maxU)
        _ctc_call(logits, None, labels, input_lengths, label_lengths, None, costs, ws, blank, maxU)
        ctx.save_for_backward(logits, labels, input_lengths, label_lengths, ws)
        ctx.args = (blank, maxU)
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        logits, labels, input_lengths, label_lengths, ws = ctx.saved_tensors
        scale = grad_costs.to(device=logits.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(logits.device):
            grads = torch.empty_like(logits)
        _ctc_call(logits, grads, labels, input_lengths, label_lengths, scale, None, ws, *ctx.args)
        return (grads,) + (None,) * 5


# ---- the float64 torch mirror (CPU) ---------------------------------------------------------------------------------------
def _lse(*xs):
    """logsumexp of float64 tensors of one shape, -inf where all are -inf."""
    x = torch.stack(xs)
    m = x.max(dim=0).values
    ms = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    return torch.where(m == _NEG_INF, m, ms + torch.log(torch.exp(x - ms).sum(dim=0)))


def _shift(a, n):
    """a moved n states up (n > 0) or down, -inf moved in."""
    pad = a.new_full((abs(n),), _NEG_INF)
    return torch.cat([pad, a])[:a.numel()] if n > 0 else torch.cat([a, pad])[-n:]


def _mirror_utterance(x, y, blank):
    """x [T, V] float64 logits, y [L] int64 -> (cost, grads [T, V]) by the rule of include/rnnt_ctc.h."""
    T, V = x.shape
    L = y.numel()
    lp = torch.log_softmax(x, dim=1)
    S = 2 * L + 1
    z = torch.full((S,), blank, dtype=torch.int64)
    z[1::2] = y
    skip = torch.zeros(S, dtype=torch.bool)  # state s may be entered from s - 2
    if L >= 2:
        skip[3::2] = y[1:] != y[:-1]
    skip_out = _shift(skip.to(torch.float64), -2) > 0  # state s may be left for s + 2
    e = lp[:, z]
    ninf = torch.full((S,), _NEG_INF, dtype=torch.float64)
    alpha = torch.full((T, S), _NEG_INF, dtype=torch.float64)
    alpha[0, :min(S, 2)] = e[0, :min(S, 2)]
    for t in range(1, T):
        a = alpha[t - 1]
        alpha[t] = e[t] + _lse(a, _shift(a, 1), torch.where(skip, _shift(a, 2), ninf))
    beta = torch.full((T, S), _NEG_INF, dtype=torch.float64)
    beta[T - 1, max(S - 2, 0):] = e[T - 1, max(S - 2, 0):]
    for t in range(T - 2, -1, -1):
        b = beta[t + 1]
        beta[t] = e[t] + _lse(b, _shift(b, -1), torch.where(skip_out, _shift(b, -2), ninf))
    lnP = _lse(alpha[T - 1, S - 1], alpha[T - 1, S - 2]) if L else alpha[T - 1, 0]
    if lnP == _NEG_INF:
        return -lnP, torch.zeros_like(x)
    occ = torch.exp(alpha + beta - e - lnP)
    return -lnP, torch.softmax(x, dim=1).index_add(1, z, -occ)


def _mirror(logits, labels, input_lengths, label_lengths, blank, cost_scale=None):
    """(costs [B], grads [B, T, V]) in float64, the library's contract: padded frames zero, invalid utterances NaN."""
    B, T, V = logits.shape
    Lmax = labels.shape[1]
    costs = torch.zeros(B, dtype=torch.float64)
    grads = torch.zeros((B, T, V), dtype=torch.float64)
    for b in range(B):
        Tb, Lb = int(input_lengths[b]), int(label_lengths[b])
        Tc, Lc = min(max(Tb, 1), T), min(max(Lb, 0), Lmax)
        y = labels[b, :Lc].to(torch.int64).clamp(0, V - 1)
        if Tb != Tc or Lb != Lc or bool((y == blank).any()):
            costs[b] = float("nan")
            grads[b, :Tc] = float("nan")
            continue
        costs[b], grads[b, :Tc] = _mirror_utterance(logits[b, :Tc].to(torch.float64), y, blank)
        if cost_scale is not None:
            grads[b] *= float(cost_scale[b])
    return costs, grads


class _CTCMirrorFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, input_lengths, label_lengths, blank):
        costs, grads = _mirror(logits.detach(), labels, input_lengths, label_lengths, blank)
        ctx.save_for_backward(grads)
        ctx.dtype = logits.dtype
        return costs.to(logits.dtype)

    @staticmethod
    def backward(ctx, grad_costs):
        (grads,) = ctx.saved_tensors
        g = torch.where(grads == 0, grads, grads * grad_costs.to(torch.float64)[:, None, None])  # (0 * inf stays 0)
        return (g.to(ctx.dtype),) + (None,) * 4


# ---- the public surface -------------------------------------------------------------------------------------------------
def _zero_inf(costs, zero_infinity):
    return torch.where(torch.isinf(costs), torch.zeros_like(costs), costs) if zero_infinity else costs


def ctc_loss(logits, labels, input_lengths, label_lengths, blank_label: int = 0, zero_infinity: bool = False):
    """Per-utterance CTC costs [B] with autograd in `logits` [B, T, V]; labels [B, L_max]."""
    labels, il, ll, blank, maxU = _inputs("ctc_loss", logits, labels, input_lengths, label_lengths, blank_label)
    if logits.is_cuda:
        costs = _CTCLossFunction.apply(logits, labels, il, ll, blank, maxU)
    else:
        costs = _CTCMirrorFunction.apply(logits, labels, il, ll, blank)
    return _zero_inf(costs, zero_infinity)


def ctc_loss_and_grad(logits, labels, input_lengths, label_lengths, blank_label: int = 0, zero_infinity: bool = False,
                      cost_scale=None):
    """(costs [B], d sum(cost_scale * costs) / d logits [B, T, V]) in one call, outside autograd."""
    labels, il, ll, blank, maxU = _inputs("ctc_loss_and_grad", logits, labels, input_lengths, label_lengths, blank_label)
    logits = logits.detach().contiguous()
    if logits.is_cuda:
        ws, costs = _device_buffers(logits, maxU)
        scale = None if cost_scale is None else cost_scale.to(device=logits.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(logits.device):
            grads = torch.empty_like(logits)
        _ctc_call(logits, grads, labels, il, ll, scale, costs, ws, blank, maxU)
    else:
        costs, grads = _mirror(logits, labels, il, ll, blank, cost_scale)
        costs, grads = costs.to(logits.dtype), grads.to(logits.dtype)
    return _zero_inf(costs, zero_infinity), grads


class CTCLoss(nn.Module):
    """ctc_loss as a module; reduction "none", "sum" or "mean" (over the utterances)."""

    def __init__(self, blank_label: int = 0, reduction: str = "none", zero_infinity: bool = False):
        super().__init__()
        if reduction not in ("none", "sum", "mean"):
            raise ValueError(f"reduction must be 'none', 'sum' or 'mean', got {reduction!r}")
        self.blank_label, self.reduction, self.zero_infinity = int(blank_label), reduction, bool(zero_infinity)

    def forward(self, logits, labels, input_lengths, label_lengths):
        costs = ctc_loss(logits, labels, input_lengths, label_lengths, self.blank_label, self.zero_infinity)
        return costs if self.reduction == "none" else costs.sum() if self.reduction == "sum" else costs.mean()


@torch.no_grad()
def ctc_greedy_decode(logits, input_lengths, blank_label: int = 0, return_frames: bool = False):
    """Best-path decoding: a_t = argmax_v logits[b, t, v] (the lowest index on ties); frame t < T_b emits a_t iff it is no blank and
    differs from a_{t-1}.  -> (tokens [B, T] int32, -1 from lengths[b] on; lengths [B] int32), and with `return_frames` the frame
    that emitted each token, in the same layout, as a third value."""
    blank = _check_logits("ctc_greedy_decode", logits, blank_label)
    B, T, V = logits.shape
    if input_lengths.numel() != B:
        raise ValueError("ctc_greedy_decode: input_lengths must be [B]")
    dev = logits.device
    il = _as_i32(input_lengths, dev).reshape(B)
    tokens = torch.empty((B, T), dtype=torch.int32, device=dev)
    frames = torch.empty((B, T), dtype=torch.int32, device=dev) if return_frames else None
    lengths = torch.empty(B, dtype=torch.int32, device=dev)
    if logits.is_cuda:
        logits = logits.detach().contiguous()
        with torch.cuda.device(dev):
            opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, blank, T, 1)
            st = _lib.load_ctc().compute_rnnt_ctc_greedy(logits.data_ptr(), il.data_ptr(), V, B, tokens.data_ptr(), ptr(frames),
                                                         lengths.data_ptr(), opts)
        _lib.check(st, "compute_rnnt_ctc_greedy")
    else:
        tokens.fill_(-1)
        if frames is not None:
            frames.fill_(-1)
        best = logits.argmax(dim=2)  # (the first of several maxima)
        for b in range(B):
            n, prev = 0, blank
            for t in range(min(max(int(il[b]), 0), T)):
                a = int(best[b, t])
                if a != blank and a != prev:
                    tokens[b, n] = a
                    if frames is not None:
                        frames[b, n] = t
                    n += 1
                prev = a
            lengths[b] = n
    return (tokens, lengths, frames) if return_frames else (tokens, lengths)
