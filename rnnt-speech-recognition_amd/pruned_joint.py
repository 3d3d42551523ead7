"""The fused joint on the pruned band: costs and gradients of the pruned transducer loss straight from the joint network's
projections (include/rnnt_pruned_joint.h compute_rnnt_joint_loss_pruned, libwarprnnt_prunedjoint.so).

pruning.py leaves the joint to the caller: gather the band's prediction rows, form tanh(a + p) @ W2 + b2 in torch, hand the logits
[B, T, S, V] to rnnt_loss_pruned.  Here the joint is inside the library, as it is for the full lattice (joint.py): neither the
logits nor the gathered rows [B, T, S, J] exist in memory.

    sb = prune_ranges(occupancy, input_lengths, label_lengths, s_range)
    costs = rnnt_joint_loss_pruned(enc_proj, pred_proj, W2, b2, sb, labels, input_lengths, label_lengths, s_range=s_range)

logits(b, t, s, :) = tanh(enc_proj[b, t] + pred_proj[b, u]) @ W2 + b2 with u = s_begin[b, t] + s; the cell is PRESENT iff t < T_b
and 0 <= u <= L_b.  An absent slot reads NO row of either projection (prune_joint_inputs clamps the row index instead), so rows
beyond an utterance's lengths may hold anything.  Everything after the logits is rnnt_loss_pruned's contract.

Device tensors run the HIP library (no eager fallback: a missing library is an error).  CPU tensors run a float64 torch mirror of
the same contract; the mirror returns float64 costs (and float64 gradients from rnnt_joint_loss_pruned_and_grad)."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import ptr
from .loss import _as_i32, check_fastemit_lambda, check_topology
from .pruning import MAX_S_RANGE, _TOPOLOGY_ID, _check_blank, _mirror as _band_mirror, prune_ranges
from .simple import rnnt_loss_simple

MAX_JOINT_SIZE = 640
MAX_ALPHABET_SIZE = 8192


# ---- arguments ----------------------------------------------------------------------------------------------------------
def _inputs(what, enc_proj, pred_proj, W2, b2, s_begin, labels, input_lengths, label_lengths, s_range, copies=True):
    """Checks and conversions: (enc, pred, W2, b2 contiguous and detached -- None without `copies`: the autograd route hands the
    caller's own tensors on --, s_begin [B, T] int32, labels [B, >= 1] int32, input_lengths, label_lengths, S)."""
    for name, x, nd in (("enc_proj", enc_proj, 3), ("pred_proj", pred_proj, 3), ("W2", W2, 2), ("b2", b2, 1)):
        if not isinstance(x, torch.Tensor) or x.dim() != nd:
            raise ValueError(f"{what}: {name} must be a tensor with {nd} dimensions")
        if x.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be float32")
        if x.device != enc_proj.device:
            raise ValueError(f"{what}: {name} must be on the device of enc_proj")
    B, T, J = enc_proj.shape
    if pred_proj.shape[0] != B or pred_proj.shape[2] != J:
        raise ValueError(f"{what}: pred_proj must be [B, U, J] = [{B}, U, {J}], got {tuple(pred_proj.shape)}")
    U = pred_proj.shape[1]
    if W2.shape[0] != J or tuple(b2.shape) != (W2.shape[1],):
        raise ValueError(f"{what}: W2 must be [J, V] = [{J}, V] and b2 [V], got {tuple(W2.shape)} and {tuple(b2.shape)}")
    V = W2.shape[1]
    if J % 64 != 0 or not 64 <= J <= MAX_JOINT_SIZE:
        raise ValueError(f"{what}: the joint size must be a multiple of 64 in 64 ... {MAX_JOINT_SIZE}, got {J}")
    if not 2 <= V <= MAX_ALPHABET_SIZE:
        raise ValueError(f"{what}: the alphabet size must be in 2 ... {MAX_ALPHABET_SIZE}, got {V}")
    if B < 1 or T < 1:
        raise ValueError(f"{what}: enc_proj must have at least one utterance and one frame")
    if s_begin.dtype.is_floating_point or s_begin.dtype == torch.bool:
        raise TypeError(f"{what}: s_begin must be an integer tensor")
    if s_begin.dim() == 3:  # k2's ranges [B, T, S]: where each band begins
        S = s_begin.shape[2] if s_range is None else int(s_range)
        if tuple(s_begin.shape) != (B, T, S):
            raise ValueError(f"{what}: s_begin must be [B, T] or [B, T, S] = [{B}, {T}, {S}], got {tuple(s_begin.shape)}")
        s_begin = s_begin[..., 0]
    elif s_begin.dim() == 2 and tuple(s_begin.shape) == (B, T):
        if s_range is None:
            raise ValueError(f"{what}: s_range is required with s_begin [B, T]")
        S = int(s_range)
    else:
        raise ValueError(f"{what}: s_begin must be [B, T] = [{B}, {T}] or [B, T, S], got {tuple(s_begin.shape)}")
    if not 1 <= S <= MAX_S_RANGE:
        raise ValueError(f"{what}: s_range (the band width) must be in 1 ... {MAX_S_RANGE}, got {S}")
    if labels.dim() != 2 or labels.shape[0] != B or labels.shape[1] != U - 1:
        raise ValueError(f"{what}: labels must be [B, U - 1] = [{B}, {U - 1}], got {tuple(labels.shape)}")
    if input_lengths.numel() != B or label_lengths.numel() != B:
        raise ValueError(f"{what}: input_lengths and label_lengths must be [B]")
    if not 1 <= U <= 8192:
        raise ValueError(f"{what}: at most 8191 labels per utterance, got {U - 1}")
    dev = enc_proj.device
    labels = _as_i32(labels, dev)
    if labels.numel() == 0:
        labels = torch.zeros((B, 1), dtype=torch.int32, device=dev)
    c = lambda x: x.detach().contiguous() if copies else None  # noqa: E731
    return (c(enc_proj), c(pred_proj), c(W2), c(b2), _as_i32(s_begin, dev), labels, _as_i32(input_lengths, dev).reshape(B),
            _as_i32(label_lengths, dev).reshape(B), S)


# ---- the device route ---------------------------------------------------------------------------------------------------
def _joint_call(enc, pred, W2, b2, sb, labels, il, ll, scale, costs, grads, ws, S, blank, lam, topology):
    """compute_rnnt_joint_loss_pruned on the current stream (scale / costs: tensors or None; grads: four tensors or None)."""
    B, T, J = enc.shape
    U, V = pred.shape[1], W2.shape[1]
    g = (None,) * 4 if grads is None else grads
    with torch.cuda.device(enc.device):
        opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, int(blank), T, U)
        st = _lib.load_prunedjoint().compute_rnnt_joint_loss_pruned(
            enc.data_ptr(), pred.data_ptr(), W2.data_ptr(), b2.data_ptr(), sb.data_ptr(), labels.data_ptr(), ll.data_ptr(),
            il.data_ptr(), ptr(scale), J, V, B, S, _TOPOLOGY_ID[topology], ptr(costs), ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]),
            ws.data_ptr(), opts, lam)
    _lib.check(st, "compute_rnnt_joint_loss_pruned")


def _buffers(enc, S):
    B, T, J = enc.shape
    with torch.cuda.device(enc.device):
        ws = torch.empty(_lib.pruned_joint_workspace_bytes(T, S, B, J), dtype=torch.uint8, device=enc.device)
        costs = torch.empty(B, dtype=torch.float32, device=enc.device)
    return ws, costs


def _grad_buffers(enc, pred, W2, b2):
    with torch.cuda.device(enc.device):
        return torch.empty_like(enc), torch.empty_like(pred), torch.empty_like(W2), torch.empty_like(b2)


class _RNNTPrunedJointFunction(torch.autograd.Function):
    """A forward-only call in forward, a gradient-only call in backward with the upstream gradient as cost_scale."""

    @staticmethod
    def forward(ctx, enc, pred, W2, b2, sb, labels, il, ll, S, blank, lam, topology):
        enc, pred, W2, b2 = enc.detach(), pred.detach(), W2.detach(), b2.detach()
        ws, costs = _buffers(enc, S)
        _joint_call(enc, pred, W2, b2, sb, labels, il, ll, None, costs, None, ws, S, blank, lam, topology)
        ctx.save_for_backward(enc, pred, W2, b2, sb, labels, il, ll, ws)
        ctx.args = (S, blank, lam, topology)
        return costs

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_costs):
        enc, pred, W2, b2, sb, labels, il, ll, ws = ctx.saved_tensors
        scale = grad_costs.to(device=enc.device, dtype=torch.float32).contiguous()
        grads = _grad_buffers(enc, pred, W2, b2)
        _joint_call(enc, pred, W2, b2, sb, labels, il, ll, scale, None, grads, ws, *ctx.args)
        return grads + (None,) * 8


# ---- the float64 torch mirror (CPU) ---------------------------------------------------------------------------------------
def _mirror(enc, pred, W2, b2, sb, labels, il, ll, S, blank, lam, topology, cost_scale=None):
    """(costs [B], d_enc_proj, d_pred_proj, dW2, db2) in float64 on the CPU.  The logits are formed for present slots alone: an
    absent slot reads no row of enc or pred."""
    B, T, J = enc.shape
    U, V = pred.shape[1], W2.shape[1]
    W, bias = W2.to(torch.float64), b2.to(torch.float64)
    Tb = il.to(torch.int64).clamp(1, T)
    Lb = ll.to(torch.int64).clamp(0, U - 1)
    u = sb.to(torch.int64)[:, :, None] + torch.arange(S, dtype=torch.int64)[None, None, :]
    present = (torch.arange(T)[None, :, None] < Tb[:, None, None]) & (u >= 0) & (u <= Lb[:, None, None])
    bb, tt, ss = torch.nonzero(present, as_tuple=True)
    uu = u[bb, tt, ss]
    h = torch.tanh(enc[bb, tt].to(torch.float64) + pred[bb, uu].to(torch.float64))  # [N, J]: the present slots alone
    acts = torch.zeros((B, T, S, V), dtype=torch.float64)
    acts[bb, tt, ss] = h @ W + bias
    costs, dl = _band_mirror(acts, sb, labels, il, ll, blank, lam, topology, U, cost_scale)
    dl = dl[bb, tt, ss]
    dz = (dl @ W.t()) * (1.0 - h * h)
    d_enc = torch.zeros((B, T, J), dtype=torch.float64)
    d_pred = torch.zeros((B, U, J), dtype=torch.float64)
    d_enc.index_put_((bb, tt), dz, accumulate=True)
    d_pred.index_put_((bb, uu), dz, accumulate=True)
    return costs, d_enc, d_pred, h.t() @ dl, dl.sum(dim=0)


class _RNNTPrunedJointMirrorFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, pred, W2, b2, sb, labels, il, ll, S, blank, lam, topology):
        ctx.inputs = (enc.detach(), pred.detach(), W2.detach(), b2.detach(), sb, labels, il, ll, S, blank, lam, topology)
        costs = _mirror(*ctx.inputs)[0]
        return costs

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_costs):
        grads = _mirror(*ctx.inputs, cost_scale=grad_costs.to(torch.float64))[1:]
        return tuple(g.to(torch.float32) for g in grads) + (None,) * 8


# ---- the public surface -------------------------------------------------------------------------------------------------
def rnnt_joint_loss_pruned(enc_proj, pred_proj, W2, b2, s_begin, labels, input_lengths, label_lengths, blank_label: int = 0,
                           fastemit_lambda: float = 0.0, topology: str = "standard", s_range: int | None = None):
    """Per-utterance transducer negative log-likelihood on a band of S symbols per frame, with the joint network inside:
    differentiable in enc_proj, pred_proj, W2 and b2.

    enc_proj [B, T, J], pred_proj [B, U, J], W2 [J, V], b2 [V] float32 (J a multiple of 64 up to 640, 2 <= V <= 8192); s_begin
    [B, T] integers (any value is legal) with s_range = S given, or k2's ranges [B, T, S], of which [..., 0] is taken; labels
    [B, U - 1]; input_lengths / label_lengths [B].  topology "standard" or "modified"; fastemit_lambda in [0, 1] scales the gradient
    through the label edges by 1 + lambda.  A band that does not connect (0, 0) to the end costs +inf, with zero gradients.  The
    forward is one forward-only call of compute_rnnt_joint_loss_pruned, the backward one gradient-only call with the upstream
    gradient as cost_scale.  Returns costs [B]: float32 on a device, float64 from the CPU mirror."""
    what = "rnnt_joint_loss_pruned"
    topology = check_topology(topology)
    lam = check_fastemit_lambda(fastemit_lambda)
    _, _, _, _, sb, labels, il, ll, S = _inputs(what, enc_proj, pred_proj, W2, b2, s_begin, labels, input_lengths, label_lengths, s_range,
                                                copies=False)
    blank = _check_blank(what, blank_label, W2.shape[1])
    fn = _RNNTPrunedJointFunction if enc_proj.is_cuda else _RNNTPrunedJointMirrorFunction
    c = lambda x: x if x.is_contiguous() else x.contiguous()  # noqa: E731
    return fn.apply(c(enc_proj), c(pred_proj), c(W2), c(b2), sb, labels, il, ll, S, blank, lam, topology)


def rnnt_joint_loss_pruned_and_grad(enc_proj, pred_proj, W2, b2, s_begin, labels, input_lengths, label_lengths, blank_label: int = 0,
                                    fastemit_lambda: float = 0.0, topology: str = "standard", s_range: int | None = None):
    """compute_rnnt_joint_loss_pruned as one combined call: (costs [B], d_enc_proj, d_pred_proj, dW2, db2), the gradients of
    sum_b cost_b (unscaled).  The arguments of rnnt_joint_loss_pruned; no autograd graph is built.  CPU tensors: the float64 mirror
    (float64 results)."""
    what = "rnnt_joint_loss_pruned_and_grad"
    topology = check_topology(topology)
    lam = check_fastemit_lambda(fastemit_lambda)
    enc, pred, W, bias, sb, labels, il, ll, S = _inputs(what, enc_proj, pred_proj, W2, b2, s_begin, labels, input_lengths,
                                                        label_lengths, s_range)
    blank = _check_blank(what, blank_label, W.shape[1])
    if not enc.is_cuda:
        return _mirror(enc, pred, W, bias, sb, labels, il, ll, S, blank, lam, topology)
    ws, costs = _buffers(enc, S)
    grads = _grad_buffers(enc, pred, W, bias)
    _joint_call(enc, pred, W, bias, sb, labels, il, ll, None, costs, grads, ws, S, blank, lam, topology)
    return (costs,) + grads


def rnnt_loss_two_pass_fused(am, lm, enc_proj, pred_proj, W2, b2, labels, input_lengths, label_lengths, s_range: int,
                             blank_label: int = 0, lm_only_scale: float = 0.0, am_only_scale: float = 0.0,
                             fastemit_lambda: float = 0.0, topology: str = "standard", ordered_ranges: bool = False):
    """simple.rnnt_loss_two_pass with the fused second pass: (simple_costs [B], pruned_costs [B], s_begin [B, T] int32).

    1. rnnt_loss_simple(am, lm, ...) -> simple_costs (differentiable in am and lm) and the occupancies;
    2. prune_ranges(occupancy, ..., s_range, ordered=ordered_ranges) -> s_begin (ordered: the rule with a defined order of
       additions, the same band on every route; on a device two launches of libwarprnnt_pruneranges.so);
    3. rnnt_joint_loss_pruned(enc_proj, pred_proj, W2, b2, s_begin, ...) -> pruned_costs, differentiable in the four: the joint
       tanh(enc_proj[b, t] + pred_proj[b, u]) @ W2 + b2 is evaluated inside the library, on the band alone."""
    lam = check_fastemit_lambda(fastemit_lambda)
    simple_costs, occ = rnnt_loss_simple(am, lm, labels, input_lengths, label_lengths, blank_label, lm_only_scale, am_only_scale,
                                         topology)
    s_begin = prune_ranges(occ, input_lengths, label_lengths, s_range, ordered=ordered_ranges)
    pruned_costs = rnnt_joint_loss_pruned(enc_proj, pred_proj, W2, b2, s_begin, labels, input_lengths, label_lengths, blank_label,
                                          lam, topology, s_range=s_range)
    return simple_costs, pruned_costs, s_begin
