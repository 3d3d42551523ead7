"""The fused TDT joint: costs and gradients of the token-and-duration (TDT) transducer loss straight from the joint network's
projections (include/rnnt_tdt_joint.h compute_rnnt_joint_loss_tdt, libwarprnnt_tdtjoint.so).

tdt.rnnt_loss_tdt leaves the joint to the caller: form tanh(a + p) @ W2 + b2 in torch and hand the logits [B, T, U, V + D] over.
Here the joint is inside the library, as it is for the transducer loss (joint.py) and the pruned band (pruned_joint.py): neither
the logits nor their gradients exist in memory.

    costs = rnnt_joint_loss_tdt(enc_proj, pred_proj, W2, b2, labels, input_lengths, label_lengths, durations=[0, 1, 2, 3, 4])

logits(b, t, u, :) = tanh(enc_proj[b, t] + pred_proj[b, u]) @ W2 + b2: the first V columns are the token head, the last
D = len(durations) the duration head.  They are formed for live cells alone (t < T_b, u <= L_b), so rows beyond an utterance's
lengths may hold anything.  Everything after the logits is rnnt_loss_tdt's contract.

Device tensors run the HIP library (no eager fallback: a missing library is an error).  CPU tensors run a float64 torch mirror of
the same contract; the mirror returns float64 costs (and float64 gradients from rnnt_joint_loss_tdt_and_grad)."""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import ptr
from .loss import _as_i32
from .tdt import MAX_U, _mirror as _lattice_mirror, check_durations, check_sigma

MAX_JOINT_SIZE = 640
MAX_LOGITS = 8192  # V + D at most


# ---- arguments ----------------------------------------------------------------------------------------------------------
def _inputs(what, enc_proj, pred_proj, W2, b2, labels, input_lengths, label_lengths, durations, blank_label, sigma, copies=True):
    """Checks and conversions: (enc, pred, W2, b2 contiguous and detached -- None without `copies`: the autograd route hands the
    caller's own tensors on --, labels [B, >= 1] int32, input_lengths, label_lengths, durations, blank, sigma)."""
    dur, sigma = check_durations(durations), check_sigma(sigma)
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
        raise ValueError(f"{what}: W2 must be [J, V + D] = [{J}, V + D] and b2 [V + D], got {tuple(W2.shape)} and {tuple(b2.shape)}")
    R = W2.shape[1]
    V = R - len(dur)
    if J % 64 != 0 or not 64 <= J <= MAX_JOINT_SIZE:
        raise ValueError(f"{what}: the joint size must be a multiple of 64 in 64 ... {MAX_JOINT_SIZE}, got {J}")
    if V < 2 or R > MAX_LOGITS:
        raise ValueError(f"{what}: W2 must have V + D = V + {len(dur)} columns with V >= 2 and V + D <= {MAX_LOGITS}, got {R}")
    if B < 1 or T < 1:
        raise ValueError(f"{what}: enc_proj must have at least one utterance and one frame")
    if not 1 <= U <= MAX_U:
        raise ValueError(f"{what}: pred_proj must have 1 ... {MAX_U} label positions, got {U}")
    if labels.dim() != 2 or labels.shape[0] != B or labels.shape[1] != U - 1 and (U, labels.shape[1]) != (1, 1):
        raise ValueError(f"{what}: labels must be [B, U - 1] = [{B}, {U - 1}], got {tuple(labels.shape)}")
    if input_lengths.numel() != B or label_lengths.numel() != B:
        raise ValueError(f"{what}: input_lengths and label_lengths must be [B]")
    blank = int(blank_label)
    if not 0 <= blank < V:
        raise ValueError(f"{what}: blank_label must be in [0, {V}), got {blank_label!r}")
    dev = enc_proj.device
    labels = _as_i32(labels, dev)
    if labels.numel() == 0:
        labels = torch.zeros((B, 1), dtype=torch.int32, device=dev)
    c = lambda x: x.detach().contiguous() if copies else None  # noqa: E731
    return (c(enc_proj), c(pred_proj), c(W2), c(b2), labels, _as_i32(input_lengths, dev).reshape(B),
            _as_i32(label_lengths, dev).reshape(B), dur, blank, sigma)


# ---- the device route ---------------------------------------------------------------------------------------------------
def _joint_call(enc, pred, W2, b2, labels, il, ll, scale, costs, grads, ws, dur, blank, sigma):
    """compute_rnnt_joint_loss_tdt on the current stream (scale / costs: tensors or None; grads: four tensors or None)."""
    B, T, J = enc.shape
    U, R = pred.shape[1], W2.shape[1]
    g = (None,) * 4 if grads is None else grads
    d = (ctypes.c_int * len(dur))(*dur)
    with torch.cuda.device(enc.device):
        opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, int(blank), T, U)
        st = _lib.load_tdtjoint().compute_rnnt_joint_loss_tdt(
            enc.data_ptr(), pred.data_ptr(), W2.data_ptr(), b2.data_ptr(), labels.data_ptr(), ll.data_ptr(), il.data_ptr(),
            ptr(scale), J, R - len(dur), d, len(dur), sigma, B, ptr(costs), ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]),
            ws.data_ptr(), opts)
    _lib.check(st, "compute_rnnt_joint_loss_tdt")


def _buffers(enc, U, D):
    B, T, J = enc.shape
    with torch.cuda.device(enc.device):
        ws = torch.empty(_lib.tdt_joint_workspace_bytes(T, U, B, D, J), dtype=torch.uint8, device=enc.device)
        costs = torch.empty(B, dtype=torch.float32, device=enc.device)
    return ws, costs


def _grad_buffers(enc, pred, W2, b2):
    with torch.cuda.device(enc.device):
        return torch.empty_like(enc), torch.empty_like(pred), torch.empty_like(W2), torch.empty_like(b2)


class _TDTJointFunction(torch.autograd.Function):
    """A forward-only call in forward, a gradient-only call in backward with the upstream gradient as cost_scale."""

    @staticmethod
    def forward(ctx, enc, pred, W2, b2, labels, il, ll, dur, blank, sigma):
        enc, pred, W2, b2 = enc.detach(), pred.detach(), W2.detach(), b2.detach()
        ws, costs = _buffers(enc, pred.shape[1], len(dur))
        _joint_call(enc, pred, W2, b2, labels, il, ll, None, costs, None, ws, dur, blank, sigma)
        ctx.save_for_backward(enc, pred, W2, b2, labels, il, ll, ws)
        ctx.args = (dur, blank, sigma)
        return costs

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_costs):
        enc, pred, W2, b2, labels, il, ll, ws = ctx.saved_tensors
        scale = grad_costs.to(device=enc.device, dtype=torch.float32).contiguous()
        grads = _grad_buffers(enc, pred, W2, b2)
        _joint_call(enc, pred, W2, b2, labels, il, ll, scale, None, grads, ws, *ctx.args)
        return grads + (None,) * 6


# ---- the float64 torch mirror (CPU) ---------------------------------------------------------------------------------------
def _mirror(enc, pred, W2, b2, labels, il, ll, dur, blank, sigma, cost_scale=None, need_grad=True):
    """(costs [B], d_enc_proj, d_pred_proj, dW2, db2) in float64 on the CPU (the gradients None without `need_grad`): the logits
    of the live cells alone (a padded cell reads no row of enc or pred), tdt._mirror on them, and the chain rule back through the
    joint.  The gradients are those of sum_b cost_scale[b] cost_b; an utterance without a path contributes zeros."""
    B, T, J = enc.shape
    U, R = pred.shape[1], W2.shape[1]
    e64, p64 = enc.detach().to(torch.float64), pred.detach().to(torch.float64)
    W, bias = W2.detach().to(torch.float64), b2.detach().to(torch.float64)
    Tb = il.to(torch.int64).clamp(1, T)
    Lb = ll.to(torch.int64).clamp(0, U - 1)
    live = (torch.arange(T)[None, :, None] < Tb[:, None, None]) & (torch.arange(U)[None, None, :] <= Lb[:, None, None])
    bb, tt, uu = torch.nonzero(live, as_tuple=True)
    h = torch.tanh(e64[bb, tt] + p64[bb, uu])  # [N, J]: the live cells alone
    x = (h @ W + bias).requires_grad_(need_grad)
    acts = torch.zeros((B, T, U, R), dtype=torch.float64).index_put((bb, tt, uu), x)
    costs = _lattice_mirror(acts, labels, il, ll, dur, blank, sigma)
    if not need_grad:
        return costs.detach(), None, None, None, None
    cs = torch.ones(B, dtype=torch.float64) if cost_scale is None else cost_scale.to(torch.float64).reshape(B)
    fin = torch.isfinite(costs) | torch.isnan(costs)  # (+inf: no path -- nothing to differentiate, its gradients are zeros)
    (dl,) = torch.autograd.grad((torch.where(fin, costs, torch.zeros_like(costs)) * cs).sum(), x)
    dz = (dl @ W.t()) * (1.0 - h * h)
    d_enc = torch.zeros((B, T, J), dtype=torch.float64)
    d_pred = torch.zeros((B, U, J), dtype=torch.float64)
    d_enc.index_put_((bb, tt), dz, accumulate=True)
    d_pred.index_put_((bb, uu), dz, accumulate=True)
    return costs.detach(), d_enc, d_pred, h.t() @ dl, dl.sum(dim=0)


class _TDTJointMirrorFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, pred, W2, b2, labels, il, ll, dur, blank, sigma):
        ctx.inputs = (enc.detach(), pred.detach(), W2.detach(), b2.detach(), labels, il, ll, dur, blank, sigma)
        with torch.enable_grad():
            return _mirror(*ctx.inputs, need_grad=False)[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_costs):
        with torch.enable_grad():
            grads = _mirror(*ctx.inputs, cost_scale=grad_costs)[1:]
        return tuple(g.to(torch.float32) for g in grads) + (None,) * 6


# ---- the public surface -------------------------------------------------------------------------------------------------
def rnnt_joint_loss_tdt(enc_proj, pred_proj, W2, b2, labels, input_lengths, label_lengths, durations, blank_label: int = 0,
                        sigma: float = 0.0):
    """Per-utterance TDT negative log-likelihood with the joint network inside: differentiable in enc_proj, pred_proj, W2 and b2.

    enc_proj [B, T, J], pred_proj [B, U, J], W2 [J, V + D], b2 [V + D] float32 (J a multiple of 64 up to 640, V >= 2,
    V + D <= 8192, D = len(durations), U <= 1024); labels [B, U - 1]; input_lengths / label_lengths [B]; durations, blank_label and
    sigma as for rnnt_loss_tdt.  An utterance without a path costs +inf, with zero gradients.  The forward is one forward-only call
    of compute_rnnt_joint_loss_tdt, the backward one gradient-only call with the upstream gradient as cost_scale.  Returns costs
    [B]: float32 on a device, float64 from the CPU mirror."""
    _, _, _, _, labels, il, ll, dur, blank, sigma = _inputs("rnnt_joint_loss_tdt", enc_proj, pred_proj, W2, b2, labels, input_lengths,
                                                            label_lengths, durations, blank_label, sigma, copies=False)
    fn = _TDTJointFunction if enc_proj.is_cuda else _TDTJointMirrorFunction
    c = lambda x: x if x.is_contiguous() else x.contiguous()  # noqa: E731
    return fn.apply(c(enc_proj), c(pred_proj), c(W2), c(b2), labels, il, ll, dur, blank, sigma)


def rnnt_joint_loss_tdt_and_grad(enc_proj, pred_proj, W2, b2, labels, input_lengths, label_lengths, durations, blank_label: int = 0,
                                 sigma: float = 0.0):
    """compute_rnnt_joint_loss_tdt as one combined call: (costs [B], d_enc_proj, d_pred_proj, dW2, db2), the gradients of
    sum_b cost_b (unscaled).  The arguments of rnnt_joint_loss_tdt; no autograd graph is kept.  CPU tensors: the float64 mirror
    (float64 results)."""
    enc, pred, W, bias, labels, il, ll, dur, blank, sigma = _inputs("rnnt_joint_loss_tdt_and_grad", enc_proj, pred_proj, W2, b2, labels,
                                                                    input_lengths, label_lengths, durations, blank_label, sigma)
    if not enc.is_cuda:
        with torch.enable_grad():
            return _mirror(enc, pred, W, bias, labels, il, ll, dur, blank, sigma)
    ws, costs = _buffers(enc, pred.shape[1], len(dur))
    grads = _grad_buffers(enc, pred, W, bias)
    _joint_call(enc, pred, W, bias, labels, il, ll, None, costs, grads, ws, dur, blank, sigma)
    return (costs,) + grads


class TDTJointLoss(torch.nn.Module):
    """The TDT loss of a model's joint network, fused: forward(joint, enc, pred, labels, input_lengths, label_lengths) -> costs [B].

    joint: any object with W1 [H, J], b1 [J], W2 [J, V + D], b2 [V + D] -- what TDTGreedyJoint and TDTBeamJoint decode with; a
    joint.JointLoss built with vocab_size = V + D qualifies.  enc [B, T, H], pred [B, U, H].  The first Dense layer runs in torch
    (enc_proj = enc @ W1 + b1, pred_proj = pred @ W1, as PrunedJointLoss forms them), the rest in rnnt_joint_loss_tdt; a J that is
    not a multiple of 64 is zero-padded, which is exact: tanh(0) = 0 meets zero rows of W2.  All six of W1, b1, W2, b2, enc and
    pred receive their gradients through autograd."""

    def __init__(self, durations, blank_label: int = 0, sigma: float = 0.0):
        super().__init__()
        self.durations = check_durations(durations)
        self.sigma = check_sigma(sigma)
        self.blank_label = int(blank_label)

    def forward(self, joint, enc, pred, labels, input_lengths, label_lengths):
        enc_proj = enc @ joint.W1 + joint.b1
        pred_proj = pred @ joint.W1
        W2 = joint.W2
        J = W2.shape[0]
        pad = -J % 64
        if pad:
            enc_proj = torch.nn.functional.pad(enc_proj, (0, pad))
            pred_proj = torch.nn.functional.pad(pred_proj, (0, pad))
            W2 = torch.nn.functional.pad(W2, (0, 0, 0, pad))
        return rnnt_joint_loss_tdt(enc_proj, pred_proj, W2, joint.b2, labels, input_lengths, label_lengths, self.durations,
                                   self.blank_label, self.sigma)
