"""The simple transducer loss: an additive joiner, logit(t, u, v) = am[t, v] + lm[u, v] (include/rnnt_simple.h
compute_rnnt_loss_simple, libwarprnnt_simple.so), and the two-pass pipeline it exists for.

It is the first pass of the pruned loss (pruning.py): from am [B, T, V] and lm [B, U, V] alone -- the [B, T, U, V] tensor is never
formed -- it gives a loss that trains the two projections and the per-cell occupancies e_b + e_l [B, T, U] that `prune_ranges`
turns into the band of the second pass.  `rnnt_loss_two_pass` is the whole pipeline:

    simple_costs, pruned_costs, s_begin = rnnt_loss_two_pass(am, lm, enc_proj, pred_proj, joint, labels, input_lengths,
                                                             label_lengths, s_range)

Edge log-probabilities, with a = am_only_scale, l = lm_only_scale, w = 1 - a - l (each of a, l, a + l in [0, 1]):
    lp(t,u,v) = w log_softmax_v(am[t] + lm[u]) + a log_softmax_v(am[t]) + l log_softmax_v(lm[u])
-- k2's smoothed interpolation without its batch-coupled unigram term; NOT bit-compatible with k2, the rule is the definition.
topology "standard" or "modified" (one symbol per frame), the lattices of rnnt_loss.  The rows am[b, t >= T_b] and
lm[b, u > L_b] are never read.  A modified utterance with more labels than frames costs +inf, with zero gradients and occupancy.

Device tensors run the HIP library (no eager fallback: a missing library is an error).  CPU tensors run a float64 torch mirror of
the same contract, so the module is usable without a device; the mirror returns float64 costs and occupancies."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import ptr
from .loss import _as_i32, check_fastemit_lambda, check_topology
from .pruning import prune_joint_inputs, prune_ranges, rnnt_loss_pruned

_TOPOLOGY_ID = {"standard": _lib.RNNT_SIMPLE_STANDARD, "modified": _lib.RNNT_SIMPLE_MODIFIED}
_NEG_INF = float("-inf")


# ---- arguments ----------------------------------------------------------------------------------------------------------
def check_simple_scales(lm_only_scale, am_only_scale):
    """(l, a) as floats; ValueError unless each of l, a and their float32 sum is finite and in [0, 1] (include/rnnt_simple.h)."""
    l, a = float(lm_only_scale), float(am_only_scale)
    ok = 0.0 <= l <= 1.0 and 0.0 <= a <= 1.0  # (NaN fails the comparisons)
    if not ok or not float(np.float32(l) + np.float32(a)) <= 1.0:
        raise ValueError(f"lm_only_scale, am_only_scale and their sum must be finite and in [0, 1], got {lm_only_scale!r}, {am_only_scale!r}")
    return l, a


def _inputs(what, am, lm, labels, input_lengths, label_lengths, blank_label, copies=True):
    """Checks and conversions: (am_c, lm_c, labels [B, >= 1] int32, input_lengths, label_lengths, blank); am_c and lm_c are detached
    and contiguous, or None without `copies` (the autograd route keeps the caller's tensors)."""
    if not isinstance(am, torch.Tensor) or not isinstance(lm, torch.Tensor) or am.dim() != 3 or lm.dim() != 3:
        raise ValueError(f"{what}: am must be [B, T, V] and lm [B, U, V]")
    if am.shape[0] != lm.shape[0] or am.shape[2] != lm.shape[2]:
        raise ValueError(f"{what}: am {tuple(am.shape)} and lm {tuple(lm.shape)} must agree in B and V")
    if am.device != lm.device or am.dtype != lm.dtype:
        raise ValueError(f"{what}: am and lm must share a device and a dtype")
    if am.dtype != torch.float32 and (am.is_cuda or am.dtype != torch.float64):
        raise TypeError(f"{what}: am and lm must be float32 (float64 as well on the CPU)")
    B, T, V = am.shape
    U = lm.shape[1]
    if T < 1 or V < 2:
        raise ValueError(f"{what}: at least one frame and two symbols, got T = {T}, V = {V}")
    if labels.dim() != 2 or labels.shape[0] != B or labels.shape[1] != U - 1 and (U, labels.shape[1]) != (1, 1):
        raise ValueError(f"{what}: labels must be [B, U - 1] = [{B}, {U - 1}], got {tuple(labels.shape)}")  # (U = 1: a column nobody reads may stand in)
    if not 1 <= U <= 8192:
        raise ValueError(f"{what}: lm must have 1 ... 8192 rows per utterance, got {U}")
    if input_lengths.numel() != B or label_lengths.numel() != B:
        raise ValueError(f"{what}: input_lengths and label_lengths must be [B]")
    blank = int(blank_label)
    if not 0 <= blank < V:
        raise ValueError(f"{what}: blank_label must be in [0, {V}), got {blank_label!r}")
    dev = am.device
    labels = _as_i32(labels, dev)
    if labels.numel() == 0:
        labels = torch.zeros((B, 1), dtype=torch.int32, device=dev)
    return (am.detach().contiguous() if copies else None, lm.detach().contiguous() if copies else None, labels, _as_i32(input_lengths, dev).reshape(B),
            _as_i32(label_lengths, dev).reshape(B), blank)


# ---- the device route ---------------------------------------------------------------------------------------------------
def _simple_call(am, lm, grad_am, grad_lm, occupancy, labels, input_lengths, label_lengths, scale, costs, ws, blank, l, a, topology):
    """compute_rnnt_loss_simple on the current stream (grad_am / grad_lm / occupancy / scale / costs: tensors or None)."""
    B, T, V = am.shape
    with torch.cuda.device(am.device):
        opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, int(blank), T, lm.shape[1])
        st = _lib.load_simple().compute_rnnt_loss_simple(
            am.data_ptr(), lm.data_ptr(), ptr(grad_am), ptr(grad_lm), ptr(occupancy), labels.data_ptr(), label_lengths.data_ptr(),
            input_lengths.data_ptr(), ptr(scale), V, B, _TOPOLOGY_ID[topology], l, a, ptr(costs), ws.data_ptr(), opts)
    _lib.check(st, "compute_rnnt_loss_simple")


def _device_buffers(am, lm):
    B, T, V = am.shape
    U = lm.shape[1]
    with torch.cuda.device(am.device):
        ws = torch.empty(_lib.simple_workspace_bytes(T, U, B), dtype=torch.uint8, device=am.device)
        costs = torch.empty(B, dtype=torch.float32, device=am.device)
        occ = torch.empty((B, T, U), dtype=torch.float32, device=am.device)
    return ws, costs, occ


class _RNNTSimpleLossFunction(torch.autograd.Function):
    """A forward-only call in forward, a gradient-only call in backward with the upstream gradient as cost_scale."""

    @staticmethod
    def forward(ctx, am, lm, labels, input_lengths, label_lengths, blank, l, a, topology):
        am, lm = am.detach(), lm.detach()
        ws, costs, occ = _device_buffers(am, lm)
        _simple_call(am, lm, None, None, occ, labels, input_lengths, label_lengths, None, costs, ws, blank, l, a, topology)
        ctx.save_for_backward(am, lm, labels, input_lengths, label_lengths, ws)
        ctx.args = (blank, l, a, topology)
        ctx.mark_non_differentiable(occ)
        return costs, occ

    @staticmethod
    def backward(ctx, grad_costs, _grad_occ):
        am, lm, labels, input_lengths, label_lengths, ws = ctx.saved_tensors
        scale = grad_costs.to(device=am.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(am.device):
            g_am, g_lm = torch.empty_like(am), torch.empty_like(lm)
        _simple_call(am, lm, g_am, g_lm, None, labels, input_lengths, label_lengths, scale, None, ws, *ctx.args)
        return (g_am, g_lm) + (None,) * 7


# ---- the float64 torch mirror (CPU) ---------------------------------------------------------------------------------------
def _lae(a, b):
    """logaddexp on float64 tensors, -inf where both are -inf."""
    m = torch.maximum(a, b)
    ms = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    return torch.where(m == _NEG_INF, m, ms + torch.log(torch.exp(a - ms) + torch.exp(b - ms)))


def _mirror_utterance(am, lm, y, blank, l, a, topology):
    """One utterance: am [T, V], lm [L + 1, V] float64 (live rows only), y [L] int64 -> (cost, occ [T, L + 1], g_am, g_lm)."""
    T, V = am.shape
    L = lm.shape[0] - 1
    w = max(0.0, 1.0 - a - l)
    x = am[:, None, :] + lm[None, :, :]
    lsj = torch.log_softmax(x, dim=-1)
    lsa, lsl = torch.log_softmax(am, dim=-1), torch.log_softmax(lm, dim=-1)
    lp = w * lsj + a * lsa[:, None, :] + l * lsl[None, :, :]
    ninf = torch.full((1,), _NEG_INF, dtype=torch.float64)
    lpb = lp[:, :, blank]
    lpl = torch.cat([lp[:, torch.arange(L), y] if L else lp[:, :0, 0], ninf.expand(T, 1)], dim=1)  # [T, L + 1], -inf at u = L
    shift = lambda row: torch.cat([ninf, row[:-1]])    # noqa: E731  (value of column u - 1)
    unshift = lambda row: torch.cat([row[1:], ninf])   # noqa: E731  (value of column u + 1)
    start = torch.full((L + 1,), _NEG_INF, dtype=torch.float64)
    start[0] = 0.0
    end = torch.full((L + 1,), _NEG_INF, dtype=torch.float64)
    end[L] = 0.0
    alpha = torch.full((T, L + 1), _NEG_INF, dtype=torch.float64)
    beta = alpha.clone()
    blank_to, label_to = alpha.clone(), alpha.clone()  # beta of the two edges' targets
    if topology == "standard":
        for t in range(T):
            row = (alpha[t - 1] + lpb[t - 1]) if t else start.clone()
            for u in range(1, L + 1):
                row[u] = _lae(row[u], row[u - 1] + lpl[t, u - 1])
            alpha[t] = row
        lnP = alpha[T - 1, L] + lpb[T - 1, L]
        for t in range(T - 1, -1, -1):
            blank_to[t] = end if t == T - 1 else beta[t + 1]
            row = lpb[t] + blank_to[t]
            for u in range(L - 1, -1, -1):
                row[u] = _lae(row[u], lpl[t, u] + row[u + 1])
            beta[t] = row
            label_to[t] = unshift(row)
    else:
        for t in range(T):
            alpha[t] = _lae(alpha[t - 1] + lpb[t - 1], shift(alpha[t - 1] + lpl[t - 1])) if t else start
        lnP = _lae(alpha[T - 1] + lpb[T - 1], shift(alpha[T - 1] + lpl[T - 1]))[L]
        for t in range(T - 1, -1, -1):
            nxt = end if t == T - 1 else beta[t + 1]
            blank_to[t], label_to[t] = nxt, unshift(nxt)
            beta[t] = _lae(lpb[t] + nxt, lpl[t] + unshift(nxt))
    if lnP == _NEG_INF:
        return torch.tensor(float("inf"), dtype=torch.float64), torch.zeros_like(alpha), torch.zeros_like(am), torch.zeros_like(lm)
    e_b = torch.exp(alpha + lpb + blank_to - lnP)
    e_l = torch.exp(alpha + lpl + label_to - lnP)
    occ = e_b + e_l
    sj = torch.exp(lsj)
    eps = torch.zeros_like(x)
    eps[:, :, blank] += e_b
    if L:
        eps[:, torch.arange(L), y] += e_l[:, :L]
    g_am = w * (occ[:, :, None] * sj).sum(1) + a * torch.exp(lsa) * occ.sum(1)[:, None] - (w + a) * eps.sum(1)
    g_lm = w * (occ[:, :, None] * sj).sum(0) + l * torch.exp(lsl) * occ.sum(0)[:, None] - (w + l) * eps.sum(0)
    return -lnP, occ, g_am, g_lm


def _mirror(am, lm, labels, input_lengths, label_lengths, blank, l, a, topology, cost_scale=None):
    """(costs [B], occupancy [B, T, U], grad_am, grad_lm) in float64 on the CPU; out-of-range lengths as the op reports them."""
    B, T, V = am.shape
    U = lm.shape[1]
    costs = torch.zeros(B, dtype=torch.float64)
    occ = torch.zeros((B, T, U), dtype=torch.float64)
    g_am = torch.zeros((B, T, V), dtype=torch.float64)
    g_lm = torch.zeros((B, U, V), dtype=torch.float64)
    for b in range(B):
        Tb, Lb = int(input_lengths[b]), int(label_lengths[b])
        bad = Tb < 1 or Tb > T or Lb < 0 or Lb > U - 1
        Tb, Lb = min(max(Tb, 1), T), min(max(Lb, 0), U - 1)
        if bad:
            costs[b] = float("nan")
            occ[b, :Tb, :Lb + 1] = float("nan")
            g_am[b, :Tb] = float("nan")
            g_lm[b, :Lb + 1] = float("nan")
            continue
        y = labels[b, :Lb].to(torch.int64).clamp(0, V - 1)
        c, o, ga, gl = _mirror_utterance(am[b, :Tb].to(torch.float64), lm[b, :Lb + 1].to(torch.float64), y, blank, l, a, topology)
        s = 1.0 if cost_scale is None else float(cost_scale[b])
        costs[b], occ[b, :Tb, :Lb + 1], g_am[b, :Tb], g_lm[b, :Lb + 1] = c, o, ga * s, gl * s
    return costs, occ, g_am, g_lm


class _RNNTSimpleMirrorFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, am, lm, labels, input_lengths, label_lengths, blank, l, a, topology):
        costs, occ, g_am, g_lm = _mirror(am.detach(), lm.detach(), labels, input_lengths, label_lengths, blank, l, a, topology)
        ctx.save_for_backward(g_am, g_lm)
        ctx.dtype = am.dtype
        ctx.mark_non_differentiable(occ)
        return costs, occ

    @staticmethod
    def backward(ctx, grad_costs, _grad_occ):
        g_am, g_lm = ctx.saved_tensors
        s = grad_costs.to(torch.float64)[:, None, None]
        return ((g_am * s).to(ctx.dtype), (g_lm * s).to(ctx.dtype)) + (None,) * 7


# ---- the public surface -------------------------------------------------------------------------------------------------
def rnnt_loss_simple(am, lm, labels, input_lengths, label_lengths, blank_label: int = 0, lm_only_scale: float = 0.0,
                     am_only_scale: float = 0.0, topology: str = "standard"):
    """(costs [B], occupancy [B, T, U]) of the additive joiner am[b, t, v] + lm[b, u, v]; costs are differentiable in `am` and `lm`.

    am [B, T, V], lm [B, U, V] float32 RAW LOGITS; labels [B, U - 1]; input_lengths / label_lengths [B].  The forward is one call
    of compute_rnnt_loss_simple, the backward one gradient-only call with the upstream gradient as cost_scale.  occupancy =
    e_b + e_l per lattice cell (0 on absent cells) is detached: it is what prune_ranges takes.  float32 on a device, float64
    from the CPU mirror."""
    topology = check_topology(topology)
    l, a = check_simple_scales(lm_only_scale, am_only_scale)
    _, _, labels, il, ll, blank = _inputs("rnnt_loss_simple", am, lm, labels, input_lengths, label_lengths, blank_label, copies=False)
    fn = _RNNTSimpleLossFunction if am.is_cuda else _RNNTSimpleMirrorFunction
    return fn.apply(am if am.is_contiguous() else am.contiguous(), lm if lm.is_contiguous() else lm.contiguous(), labels, il, ll,
                    blank, l, a, topology)


def rnnt_loss_simple_and_grad(am, lm, labels, input_lengths, label_lengths, blank_label: int = 0, lm_only_scale: float = 0.0,
                              am_only_scale: float = 0.0, topology: str = "standard"):
    """compute_rnnt_loss_simple as one combined call: (costs [B], occupancy [B, T, U], grad_am [B, T, V], grad_lm [B, U, V]) with
    the gradients of cost_b (unscaled).  The arguments of rnnt_loss_simple; no autograd graph is built.  CPU tensors: the float64
    mirror (float64 results)."""
    topology = check_topology(topology)
    l, a = check_simple_scales(lm_only_scale, am_only_scale)
    am_c, lm_c, labels, il, ll, blank = _inputs("rnnt_loss_simple_and_grad", am, lm, labels, input_lengths, label_lengths, blank_label)
    if not am_c.is_cuda:
        return _mirror(am_c, lm_c, labels, il, ll, blank, l, a, topology)
    ws, costs, occ = _device_buffers(am_c, lm_c)
    with torch.cuda.device(am_c.device):
        g_am, g_lm = torch.empty_like(am_c), torch.empty_like(lm_c)
    _simple_call(am_c, lm_c, g_am, g_lm, occ, labels, il, ll, None, costs, ws, blank, l, a, topology)
    return costs, occ, g_am, g_lm


def rnnt_loss_two_pass(am, lm, enc_proj, pred_proj, joint, labels, input_lengths, label_lengths, s_range: int,
                       blank_label: int = 0, lm_only_scale: float = 0.0, am_only_scale: float = 0.0,
                       fastemit_lambda: float = 0.0, topology: str = "standard", ordered_ranges: bool = False):
    """The two-pass pruned loss on one topology: (simple_costs [B], pruned_costs [B], s_begin [B, T] int32).

    1. rnnt_loss_simple(am, lm, ...) -> simple_costs (differentiable in am and lm) and the occupancies;
    2. prune_ranges(occupancy, ..., s_range, ordered=ordered_ranges) -> s_begin, where each frame's band of s_range symbols begins;
    3. prune_joint_inputs(enc_proj [B, T, J], pred_proj [B, U, J], s_begin, s_range) -> (a [B, T, 1, J], p [B, T, S, J]);
    4. joint(a, p) -> the band's logits [B, T, S, V] float32 (the caller's joint, e.g. lambda a, p: torch.tanh(a + p) @ W2 + b2);
    5. rnnt_loss_pruned(logits, s_begin, ..., fastemit_lambda) -> pruned_costs (differentiable in enc_proj, pred_proj and
       whatever the joint closes over).
    A training loss is a weighted sum of the two costs, as in k2's recipes."""
    lam = check_fastemit_lambda(fastemit_lambda)
    simple_costs, occ = rnnt_loss_simple(am, lm, labels, input_lengths, label_lengths, blank_label, lm_only_scale,
                                         am_only_scale, topology)
    s_begin = prune_ranges(occ, input_lengths, label_lengths, s_range, ordered=ordered_ranges)
    a, p = prune_joint_inputs(enc_proj, pred_proj, s_begin, s_range)
    pruned_costs = rnnt_loss_pruned(joint(a, p), s_begin, labels, input_lengths, label_lengths, blank_label, lam, topology)
    return simple_costs, pruned_costs, s_begin
