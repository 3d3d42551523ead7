"""Host-side mirror of the reference's loss surface, on PyTorch-ROCm over the C ABI.

Reference interface (same names, argument order and meaning):
  utils/loss.py:12-38   get_loss_fn(reduction_factor) -> _loss_fn(y_true, y_pred, spec_lengths, label_lengths)
  utils/loss.py:6,34-35 warprnnt_tensorflow.rnnt_loss(acts, labels, input_lengths, label_lengths, blank_label=0)
Call sites: run_rnnt.py:493-494 (construction), :272-273 (positional), :405-407 (keywords).

Differences, all deliberate:
  * the native op is libwarprnnt.so for gfx950 (include/rnnt.h); PyTorch only provides device
    memory, the HIP stream and autograd plumbing;
  * there is no silent fallback (utils/loss.py:14-22 returns the logits when the op is missing):
    a missing library or a CPU tensor raises;
  * the gradient pass runs in backward() with the upstream gradient folded in
    (compute_rnnt_loss_bwd), instead of computing unscaled grads in forward and multiplying later.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._lib import ptr


def _as_i32(x: torch.Tensor, device) -> torch.Tensor:
    return x.to(device=device, dtype=torch.int32).contiguous()


def check_fastemit_lambda(fastemit_lambda) -> float:
    """FastEmit's weight as a float; ValueError unless it is finite and in [0, 1] (include/rnnt.h compute_rnnt_loss_fastemit)."""
    lam = float(fastemit_lambda)
    if not (0.0 <= lam <= 1.0):  # (NaN fails both comparisons)
        raise ValueError(f"fastemit_lambda must be finite and in [0, 1], got {fastemit_lambda!r}")
    return lam


class _RNNTLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, acts, labels, input_lengths, label_lengths, blank_label, fastemit_lambda=0.0):
        lib = _lib.load()
        if not acts.is_cuda:
            raise RuntimeError(
                "rnnt_loss: acts must live on an MI355X (cuda/HIP) device; this engine has no CPU path"
            )
        if acts.dim() != 4:
            raise ValueError("rnnt_loss: acts must be [B, T, U, V]")
        if acts.dtype != torch.float32:
            raise TypeError("rnnt_loss: acts must be float32 (the reference op is float32-only)")
        B, T, U, V = acts.shape
        dev = acts.device
        acts_c = acts.detach().contiguous()
        labels = _as_i32(labels, dev)
        input_lengths = _as_i32(input_lengths, dev)
        label_lengths = _as_i32(label_lengths, dev)
        if U > 1 and tuple(labels.shape) != (B, U - 1):
            raise ValueError(f"rnnt_loss: labels must be [B, U-1] = [{B}, {U - 1}], got {tuple(labels.shape)}")
        if input_lengths.numel() != B or label_lengths.numel() != B:
            raise ValueError("rnnt_loss: input_lengths and label_lengths must be [B]")
        if labels.numel() == 0:
            labels = torch.zeros((B, 1), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            ws = torch.empty(_lib.workspace_bytes(T, U, B), dtype=torch.uint8, device=dev)
            costs = torch.empty(B, dtype=torch.float32, device=dev)
            opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, int(blank_label), T, U)
            st = lib.compute_rnnt_loss_fwd(
                acts_c.data_ptr(), labels.data_ptr(), label_lengths.data_ptr(), input_lengths.data_ptr(),
                V, B, costs.data_ptr(), ws.data_ptr(), opts)
        _lib.check(st, "compute_rnnt_loss_fwd")
        ctx.save_for_backward(acts_c, labels, input_lengths, label_lengths, ws)
        ctx.blank = int(blank_label)
        ctx.fastemit_lambda = float(fastemit_lambda)
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        acts, labels, input_lengths, label_lengths, ws = ctx.saved_tensors
        lib = _lib.load()
        B, T, U, V = acts.shape
        dev = acts.device
        scale = grad_costs.to(device=dev, dtype=torch.float32).contiguous()
        with torch.cuda.device(dev):
            grads = torch.empty_like(acts)
            opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, ctx.blank, T, U)
            if ctx.fastemit_lambda != 0.0:  # costs == NULL: the gradient pass alone, with FastEmit's weight on the label edges
                st = lib.compute_rnnt_loss_fastemit(
                    acts.data_ptr(), grads.data_ptr(), labels.data_ptr(), label_lengths.data_ptr(),
                    input_lengths.data_ptr(), scale.data_ptr(), V, B, None, ws.data_ptr(), opts, 0, ctx.fastemit_lambda)
            else:
                st = lib.compute_rnnt_loss_bwd(
                    acts.data_ptr(), grads.data_ptr(), labels.data_ptr(), label_lengths.data_ptr(),
                    input_lengths.data_ptr(), scale.data_ptr(), V, B, ws.data_ptr(), opts)
        _lib.check(st, "compute_rnnt_loss_bwd")
        return grads, None, None, None, None, None


TOPOLOGIES = ("standard", "modified")


def check_topology(topology) -> str:
    """'standard' (the Graves lattice: a label edge stays on its frame) or 'modified' (one symbol per frame: the paths the beam
    searches of decoding.py produce; include/rnnt_modified.h compute_rnnt_loss_modified); ValueError otherwise."""
    if topology not in TOPOLOGIES:
        raise ValueError(f"topology must be one of {TOPOLOGIES}, got {topology!r}")
    return topology


def _modified_inputs(what, acts, labels, input_lengths, label_lengths):
    """The checks and conversions of the standard route, for the modified op: (acts_c, labels, input_lengths, label_lengths)."""
    _lib.load()
    if not acts.is_cuda:
        raise RuntimeError(f"{what}: acts must live on an MI355X (cuda/HIP) device; this engine has no CPU path")
    if acts.dim() != 4:
        raise ValueError(f"{what}: acts must be [B, T, U, V]")
    if acts.dtype != torch.float32:
        raise TypeError(f"{what}: acts must be float32 (the reference op is float32-only)")
    B, T, U, V = acts.shape
    dev = acts.device
    labels = _as_i32(labels, dev)
    input_lengths = _as_i32(input_lengths, dev)
    label_lengths = _as_i32(label_lengths, dev)
    if U > 1 and tuple(labels.shape) != (B, U - 1):
        raise ValueError(f"{what}: labels must be [B, U-1] = [{B}, {U - 1}], got {tuple(labels.shape)}")
    if input_lengths.numel() != B or label_lengths.numel() != B:
        raise ValueError(f"{what}: input_lengths and label_lengths must be [B]")
    if labels.numel() == 0:
        labels = torch.zeros((B, 1), dtype=torch.int32, device=dev)
    return acts.detach().contiguous(), labels, input_lengths, label_lengths


def _modified_call(acts, grads, labels, input_lengths, label_lengths, scale, costs, ws, blank, lam):
    """compute_rnnt_loss_modified on the current stream (grads / scale / costs: tensors or None)."""
    B, T, U, V = acts.shape
    with torch.cuda.device(acts.device):
        opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, int(blank), T, U)
        st = _lib.load_mod().compute_rnnt_loss_modified(
            acts.data_ptr(), ptr(grads), labels.data_ptr(), label_lengths.data_ptr(), input_lengths.data_ptr(), ptr(scale),
            V, B, ptr(costs), ws.data_ptr(), opts, lam)
    _lib.check(st, "compute_rnnt_loss_modified")


class _RNNTModifiedLossFunction(torch.autograd.Function):
    """The modified topology: a forward-only call in forward, a gradient-only call in backward with the upstream gradient as
    cost_scale and FastEmit's weight passed through."""

    @staticmethod
    def forward(ctx, acts, labels, input_lengths, label_lengths, blank_label, fastemit_lambda=0.0):
        acts_c, labels, input_lengths, label_lengths = _modified_inputs("rnnt_loss", acts, labels, input_lengths, label_lengths)
        B, T, U, V = acts_c.shape
        with torch.cuda.device(acts_c.device):
            ws = torch.empty(_lib.modified_workspace_bytes(T, U, B), dtype=torch.uint8, device=acts_c.device)
            costs = torch.empty(B, dtype=torch.float32, device=acts_c.device)
        _modified_call(acts_c, None, labels, input_lengths, label_lengths, None, costs, ws, blank_label, float(fastemit_lambda))
        ctx.save_for_backward(acts_c, labels, input_lengths, label_lengths, ws)
        ctx.blank = int(blank_label)
        ctx.fastemit_lambda = float(fastemit_lambda)
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        acts, labels, input_lengths, label_lengths, ws = ctx.saved_tensors
        scale = grad_costs.to(device=acts.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(acts.device):
            grads = torch.empty_like(acts)
        _modified_call(acts, grads, labels, input_lengths, label_lengths, scale, None, ws, ctx.blank, ctx.fastemit_lambda)
        return grads, None, None, None, None, None


def rnnt_loss(acts, labels, input_lengths, label_lengths, blank_label: int = 0, fastemit_lambda: float = 0.0,
              topology: str = "standard"):
    """Per-utterance transducer negative log-likelihood, differentiable in `acts`.

    fastemit_lambda in [0, 1]: FastEmit regularisation -- the gradient through the lattice's label edges is scaled by
    1 + fastemit_lambda (typical 1e-3 ... 1e-2); the returned costs do not depend on it.

    Same contract as warprnnt_tensorflow.rnnt_loss on a CUDA build (utils/loss.py:34-35):
    acts are RAW LOGITS [B, T, U, V] (the log-softmax is fused), labels [B, U-1] int,
    input_lengths / label_lengths [B] int; returns costs [B] float32.

    topology: "standard" (the contract above) or "modified" -- every frame emits exactly one of {blank, next label}, the lattice
    of the paths the beam searches produce (include/rnnt_modified.h compute_rnnt_loss_modified); an utterance with more labels than frames
    then costs +inf and has zero gradients."""
    if check_topology(topology) == "modified":
        return _RNNTModifiedLossFunction.apply(acts, labels, input_lengths, label_lengths, blank_label,
                                               check_fastemit_lambda(fastemit_lambda))
    return _RNNTLossFunction.apply(acts, labels, input_lengths, label_lengths, blank_label, check_fastemit_lambda(fastemit_lambda))


def rnnt_loss_and_grad(acts, labels, input_lengths, label_lengths, blank_label: int = 0, visit_all: bool = False,
                       fastemit_lambda: float = 0.0, topology: str = "standard"):
    """The upstream C entry point as one call: compute_rnnt_loss(acts, grads, ...) ->
    (costs [B], grads [B,T,U,V]) with grads = d cost_b / d acts (unscaled), like the two outputs of
    the reference's WarpRNNT op.  No autograd graph is built.
    visit_all: compute_rnnt_loss_flags(..., RNNT_VISIT_ALL) -- no occupancy floor (vocabularies above 60 symbols otherwise
    write zeros for cells whose occupancy is below 2^-50 without reading their logits).
    fastemit_lambda in [0, 1]: compute_rnnt_loss_fastemit -- FastEmit's gradients (the costs do not change).
    topology "modified": compute_rnnt_loss_modified in one call; it has no occupancy floor, so visit_all with it is a ValueError."""
    lam = check_fastemit_lambda(fastemit_lambda)
    if check_topology(topology) == "modified":
        if visit_all:
            raise ValueError("rnnt_loss_and_grad: visit_all does not apply to topology='modified' (the modified op has no occupancy floor)")
        acts_c, labels, input_lengths, label_lengths = _modified_inputs("rnnt_loss_and_grad", acts, labels, input_lengths,
                                                                        label_lengths)
        B, T, U, V = acts_c.shape
        with torch.cuda.device(acts_c.device):
            ws = torch.empty(_lib.modified_workspace_bytes(T, U, B), dtype=torch.uint8, device=acts_c.device)
            costs = torch.empty(B, dtype=torch.float32, device=acts_c.device)
            grads = torch.empty_like(acts_c)
        _modified_call(acts_c, grads, labels, input_lengths, label_lengths, None, costs, ws, blank_label, lam)
        return costs, grads
    lib = _lib.load()
    if not acts.is_cuda:
        raise RuntimeError("rnnt_loss_and_grad: acts must live on an MI355X (cuda/HIP) device")
    if acts.dtype != torch.float32 or acts.dim() != 4:
        raise TypeError("rnnt_loss_and_grad: acts must be float32 [B, T, U, V]")
    B, T, U, V = acts.shape
    dev = acts.device
    acts_c = acts.detach().contiguous()
    labels = _as_i32(labels, dev)
    if labels.numel() == 0:
        labels = torch.zeros((B, 1), dtype=torch.int32, device=dev)
    input_lengths = _as_i32(input_lengths, dev)
    label_lengths = _as_i32(label_lengths, dev)
    with torch.cuda.device(dev):
        ws = torch.empty(_lib.workspace_bytes(T, U, B), dtype=torch.uint8, device=dev)
        costs = torch.empty(B, dtype=torch.float32, device=dev)
        grads = torch.empty_like(acts_c)
        opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, int(blank_label), T, U)
        if lam != 0.0:
            st = lib.compute_rnnt_loss_fastemit(
                acts_c.data_ptr(), grads.data_ptr(), labels.data_ptr(), label_lengths.data_ptr(),
                input_lengths.data_ptr(), None, V, B, costs.data_ptr(), ws.data_ptr(), opts,
                _lib.RNNT_VISIT_ALL if visit_all else 0, lam)
        elif visit_all:
            st = lib.compute_rnnt_loss_flags(
                acts_c.data_ptr(), grads.data_ptr(), labels.data_ptr(), label_lengths.data_ptr(),
                input_lengths.data_ptr(), None, V, B, costs.data_ptr(), ws.data_ptr(), opts, _lib.RNNT_VISIT_ALL)
        else:
            st = lib.compute_rnnt_loss(
                acts_c.data_ptr(), grads.data_ptr(), labels.data_ptr(), label_lengths.data_ptr(),
                input_lengths.data_ptr(), V, B, costs.data_ptr(), ws.data_ptr(), opts)
    _lib.check(st, "compute_rnnt_loss")
    return costs, grads


class RNNTLoss(torch.nn.Module):
    """nn.Module wrapper; reduction 'none' returns the reference's per-utterance costs."""

    def __init__(self, blank_label: int = 0, reduction: str = "none", fastemit_lambda: float = 0.0, topology: str = "standard"):
        super().__init__()
        self.fastemit_lambda = check_fastemit_lambda(fastemit_lambda)
        self.topology = check_topology(topology)
        if reduction not in ("none", "sum", "mean"):
            raise ValueError(reduction)
        self.blank_label = blank_label
        self.reduction = reduction

    def forward(self, acts, labels, input_lengths, label_lengths):
        costs = rnnt_loss(acts, labels, input_lengths, label_lengths, self.blank_label, self.fastemit_lambda, self.topology)
        if self.reduction == "sum":
            return costs.sum()
        if self.reduction == "mean":
            return costs.mean()
        return costs


def reduced_lengths(spec_lengths: torch.Tensor, reduction_factor) -> torch.Tensor:
    """T_b = ceil(spec_length_b / reduction_factor) as int32 (utils/loss.py:31-33)."""
    return torch.ceil(spec_lengths.to(torch.float64) / float(reduction_factor)).to(torch.int32)


def get_loss_fn(reduction_factor, topology: str = "standard"):
    """Mirror of utils/loss.py:12-38.  Returns fn(y_true, y_pred, spec_lengths, label_lengths) -> costs [B].
    topology: rnnt_loss's ("standard", the reference's lattice, or "modified").

    y_true: labels [B, U-1]; y_pred: joint logits [B, T', U, V]; spec_lengths: encoder input
    lengths BEFORE time reduction; label_lengths [B].  The reference log-softmaxes first only on
    non-CUDA builds (utils/loss.py:29-30); here the fused-softmax device op is the only path, so a
    CPU tensor raises instead of silently training on garbage."""
    if reduction_factor is None or float(reduction_factor) <= 0 or math.isnan(float(reduction_factor)):
        raise ValueError("reduction_factor must be positive")
    check_topology(topology)
    _lib.load()  # fail at construction time (run_rnnt.py:493-494), not at the first step

    def _loss_fn(y_true, y_pred, spec_lengths, label_lengths):
        y_true = y_true.to(torch.int32)
        spec_lengths = reduced_lengths(spec_lengths, reduction_factor)
        return rnnt_loss(y_pred, y_true, spec_lengths, label_lengths, topology=topology)

    return _loss_fn
