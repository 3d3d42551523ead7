"""The pruned transducer loss: loss and gradients on a band of S symbols per frame (include/rnnt_pruned.h
compute_rnnt_loss_pruned, libwarprnnt_pruned.so), and the torch plumbing around it.

A cheap first pass of the caller's gives per-cell occupancies [B, T, U]; `prune_ranges` turns them into where each frame's band
begins, `prune_joint_inputs` gathers the joint's inputs for the band, the caller forms the band's logits [B, T, S, V] with its own
joint (in torch: tanh(a + p) @ W2 + b2), and `rnnt_loss_pruned` is the loss on them, on the "standard" or the "modified" (one
symbol per frame) lattice, with FastEmit's gradients.

    sb = prune_ranges(occupancy, input_lengths, label_lengths, s_range)
    a, p = prune_joint_inputs(enc_proj, pred_proj, sb, s_range)
    costs = rnnt_loss_pruned(torch.tanh(a + p) @ W2 + b2, sb, labels, input_lengths, label_lengths)

simple.py has the first pass that produces the occupancies (rnnt_loss_simple, an additive joiner) and the whole pipeline as one
function (rnnt_loss_two_pass).

acts[b, t, s, :] are the logits of lattice cell (t, u), u = s_begin[b, t] + s; the cell is PRESENT iff t < T_b and 0 <= u <= L_b,
everything else is absent: no edges, exact-zero gradients, logits never read.  Any int32 is a legal s_begin value; a band that does
not connect (0, 0) to the end costs +inf and has zero gradients.

Device tensors run the HIP library (no eager fallback: a missing library is an error).  CPU tensors run a float64 torch mirror of
the same contract, so the module is usable without a device; the mirror returns float64 costs (and float64 gradients from
rnnt_loss_pruned_and_grad)."""
from __future__ import annotations

import torch

from . import _lib
from ._lib import ptr
from .loss import _as_i32, check_fastemit_lambda, check_topology

MAX_S_RANGE = 64
_TOPOLOGY_ID = {"standard": _lib.RNNT_PRUNED_STANDARD, "modified": _lib.RNNT_PRUNED_MODIFIED}
_NEG_INF = float("-inf")


# ---- arguments ----------------------------------------------------------------------------------------------------------
def _inputs(what, acts, s_begin, labels, input_lengths, label_lengths):
    """Checks and conversions: (acts_c, s_begin [B, T] int32, labels [B, >= 1] int32, input_lengths, label_lengths, maxU)."""
    if not isinstance(acts, torch.Tensor) or acts.dim() != 4:
        raise ValueError(f"{what}: acts must be [B, T, S, V]")
    if acts.dtype != torch.float32:
        raise TypeError(f"{what}: acts must be float32")
    B, T, S, V = acts.shape
    if not 1 <= S <= MAX_S_RANGE:
        raise ValueError(f"{what}: acts.shape[2] (the band width) must be in 1 ... {MAX_S_RANGE}, got {S}")
    if s_begin.dim() == 3:  # k2's ranges [B, T, S]: where each band begins
        if tuple(s_begin.shape) != (B, T, S):
            raise ValueError(f"{what}: s_begin must be [B, T] or [B, T, S] = [{B}, {T}, {S}], got {tuple(s_begin.shape)}")
        s_begin = s_begin[..., 0]
    elif s_begin.dim() != 2 or tuple(s_begin.shape) != (B, T):
        raise ValueError(f"{what}: s_begin must be [B, T] = [{B}, {T}] or [B, T, S], got {tuple(s_begin.shape)}")
    if s_begin.dtype.is_floating_point or s_begin.dtype == torch.bool:
        raise TypeError(f"{what}: s_begin must be an integer tensor")
    if labels.dim() != 2 or labels.shape[0] != B:
        raise ValueError(f"{what}: labels must be [B, L_max] = [{B}, ...], got {tuple(labels.shape)}")
    if input_lengths.numel() != B or label_lengths.numel() != B:
        raise ValueError(f"{what}: input_lengths and label_lengths must be [B]")
    dev = acts.device
    maxU = labels.shape[1] + 1
    if maxU > 8192:
        raise ValueError(f"{what}: at most 8191 labels per utterance, got {maxU - 1}")
    labels = _as_i32(labels, dev)
    if labels.numel() == 0:
        labels = torch.zeros((B, 1), dtype=torch.int32, device=dev)
    return (acts.detach().contiguous(), _as_i32(s_begin, dev), labels, _as_i32(input_lengths, dev).reshape(B),
            _as_i32(label_lengths, dev).reshape(B), maxU)


def _check_blank(what, blank_label, V):
    blank = int(blank_label)
    if not 0 <= blank < V:
        raise ValueError(f"{what}: blank_label must be in [0, {V}), got {blank_label!r}")
    return blank


# ---- the device route ---------------------------------------------------------------------------------------------------
def _pruned_call(acts, grads, s_begin, labels, input_lengths, label_lengths, scale, costs, ws, blank, lam, topology, maxU):
    """compute_rnnt_loss_pruned on the current stream (grads / scale / costs: tensors or None)."""
    B, T, S, V = acts.shape
    with torch.cuda.device(acts.device):
        opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, int(blank), T, maxU)
        st = _lib.load_pruned().compute_rnnt_loss_pruned(
            acts.data_ptr(), ptr(grads), s_begin.data_ptr(), labels.data_ptr(), label_lengths.data_ptr(), input_lengths.data_ptr(),
            ptr(scale), V, B, S, _TOPOLOGY_ID[topology], ptr(costs), ws.data_ptr(), opts, lam)
    _lib.check(st, "compute_rnnt_loss_pruned")


class _RNNTPrunedLossFunction(torch.autograd.Function):
    """A forward-only call in forward, a gradient-only call in backward with the upstream gradient as cost_scale."""

    @staticmethod
    def forward(ctx, acts, s_begin, labels, input_lengths, label_lengths, blank, lam, topology, maxU):
        B, T, S, V = acts.shape
        acts = acts.detach()
        with torch.cuda.device(acts.device):
            ws = torch.empty(_lib.pruned_workspace_bytes(T, S, B), dtype=torch.uint8, device=acts.device)
            costs = torch.empty(B, dtype=torch.float32, device=acts.device)
        _pruned_call(acts, None, s_begin, labels, input_lengths, label_lengths, None, costs, ws, blank, lam, topology, maxU)
        ctx.save_for_backward(acts, s_begin, labels, input_lengths, label_lengths, ws)
        ctx.args = (blank, lam, topology, maxU)
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        acts, s_begin, labels, input_lengths, label_lengths, ws = ctx.saved_tensors
        scale = grad_costs.to(device=acts.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(acts.device):
            grads = torch.empty_like(acts)
        _pruned_call(acts, grads, s_begin, labels, input_lengths, label_lengths, scale, None, ws, *ctx.args)
        return (grads,) + (None,) * 8


# ---- the float64 torch mirror (CPU) ---------------------------------------------------------------------------------------
def _lae(a, b):
    """logaddexp on float64 tensors, -inf where both are -inf."""
    m = torch.maximum(a, b)
    ms = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    return torch.where(m == _NEG_INF, m, ms + torch.log(torch.exp(a - ms) + torch.exp(b - ms)))


def _mirror_utterance(x, sb, y, T, L, blank, lam, topology):
    """One utterance: x [maxT, S, V] float64, sb [maxT] int64, y [>= L] int64 -> (cost, grads [maxT, S, V]).  The band is laid
    out on the lattice's own columns (absent cells: -inf, their alpha and beta too) and both recurrences go over it row by row."""
    maxT, S, V = x.shape
    u = sb[:, None] + torch.arange(S, dtype=torch.int64)[None, :]
    present = (torch.arange(maxT)[:, None] < T) & (u >= 0) & (u <= L)
    grads = torch.zeros_like(x)
    tt, ss = torch.nonzero(present, as_tuple=True)
    if tt.numel() == 0:
        return torch.tensor(float("inf"), dtype=torch.float64), grads
    uu = u[tt, ss]
    lp = torch.log_softmax(x[tt, ss], dim=-1)  # the present cells alone: absent logits are never read
    ninf = torch.full((T, L + 1), _NEG_INF, dtype=torch.float64)
    lpb, lpl = ninf.clone(), ninf.clone()
    pres = torch.zeros((T, L + 1), dtype=torch.bool)
    pres[tt, uu] = True
    lpb[tt, uu] = lp[:, blank]
    has = uu < L
    lab = torch.zeros_like(uu)
    if L > 0:
        lab[has] = y[uu[has]].clamp(0, V - 1)
        lpl[tt[has], uu[has]] = lp[has, lab[has]]
    mask = lambda row, t: torch.where(pres[t], row, ninf[0])  # noqa: E731
    shift = lambda row: torch.cat([ninf[0, :1], row[:-1]])    # noqa: E731  (value of column u - 1)
    unshift = lambda row: torch.cat([row[1:], ninf[0, :1]])   # noqa: E731  (value of column u + 1)
    alpha, beta = ninf.clone(), ninf.clone()
    if topology == "standard":
        for t in range(T):
            row = alpha[t - 1] + lpb[t - 1] if t else ninf[0].clone()
            if t == 0:
                row[0] = 0.0
            row = mask(row, t)
            for k in range(1, L + 1):
                if pres[t, k]:
                    row[k] = _lae(row[k], row[k - 1] + lpl[t, k - 1])
            alpha[t] = row
        lnP = alpha[T - 1, L] + lpb[T - 1, L]
        blank_to = torch.full((T, L + 1), _NEG_INF, dtype=torch.float64)  # beta of the blank edge's target
        for t in range(T - 1, -1, -1):
            if t == T - 1:
                blank_to[t, L] = 0.0
            else:
                blank_to[t] = beta[t + 1]
            row = mask(lpb[t] + blank_to[t], t)
            for k in range(L - 1, -1, -1):
                if pres[t, k]:
                    row[k] = _lae(row[k], lpl[t, k] + row[k + 1])
            beta[t] = row
        label_to = torch.stack([unshift(beta[t]) for t in range(T)])
    else:
        end = ninf[0].clone()
        end[L] = 0.0
        blank_to, label_to = ninf.clone(), ninf.clone()
        for t in range(T):
            if t == 0:
                row = ninf[0].clone()
                row[0] = 0.0
            else:
                row = _lae(alpha[t - 1] + lpb[t - 1], shift(alpha[t - 1] + lpl[t - 1]))
            alpha[t] = mask(row, t)
        lnP = _lae(alpha[T - 1] + lpb[T - 1], shift(alpha[T - 1] + lpl[T - 1]))[L]
        for t in range(T - 1, -1, -1):
            nxt = end if t == T - 1 else beta[t + 1]
            blank_to[t], label_to[t] = nxt, unshift(nxt)
            beta[t] = mask(_lae(lpb[t] + nxt, lpl[t] + unshift(nxt)), t)
    if lnP == _NEG_INF:
        return torch.tensor(float("inf"), dtype=torch.float64), grads
    e_b = torch.exp(alpha + lpb + blank_to - lnP)[tt, uu]
    e_l = torch.exp(alpha + lpl + label_to - lnP)[tt, uu]
    g = (e_b + (1.0 + lam) * e_l)[:, None] * torch.exp(lp)
    g[:, blank] -= e_b
    rows = torch.nonzero(has, as_tuple=True)[0]
    g[rows, lab[rows]] -= (1.0 + lam) * e_l[rows]
    grads[tt, ss] = g
    return -lnP, grads


def _mirror(acts, s_begin, labels, input_lengths, label_lengths, blank, lam, topology, maxU, cost_scale=None):
    """(costs [B], grads [B, T, S, V]) in float64 on the CPU; out-of-range lengths as the op reports them (NaN)."""
    B, T, S, V = acts.shape
    x = acts.to(torch.float64)
    sb = s_begin.to(torch.int64)
    costs = torch.zeros(B, dtype=torch.float64)
    grads = torch.zeros_like(x)
    for b in range(B):
        Tb, Lb = int(input_lengths[b]), int(label_lengths[b])
        bad = Tb < 1 or Tb > T or Lb < 0 or Lb > maxU - 1
        Tb, Lb = min(max(Tb, 1), T), min(max(Lb, 0), maxU - 1)
        if bad:
            u = sb[b, :, None] + torch.arange(S, dtype=torch.int64)[None, :]
            present = (torch.arange(T)[:, None] < Tb) & (u >= 0) & (u <= Lb)
            costs[b] = float("nan")
            grads[b][present] = float("nan")
            continue
        c, g = _mirror_utterance(x[b], sb[b], labels[b].to(torch.int64), Tb, Lb, blank, lam, topology)
        costs[b] = c
        grads[b] = g if cost_scale is None else g * cost_scale[b]
    return costs, grads


class _RNNTPrunedMirrorFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, acts, s_begin, labels, input_lengths, label_lengths, blank, lam, topology, maxU):
        costs, grads = _mirror(acts.detach(), s_begin, labels, input_lengths, label_lengths, blank, lam, topology, maxU)
        ctx.save_for_backward(grads)
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        (grads,) = ctx.saved_tensors
        return ((grads * grad_costs.to(torch.float64)[:, None, None, None]).to(torch.float32),) + (None,) * 8


# ---- the public surface -------------------------------------------------------------------------------------------------
def rnnt_loss_pruned(acts, s_begin, labels, input_lengths, label_lengths, blank_label: int = 0, fastemit_lambda: float = 0.0,
                     topology: str = "standard"):
    """Per-utterance transducer negative log-likelihood on a band of S symbols per frame, differentiable in `acts`.

    acts [B, T, S, V] float32 RAW LOGITS of the cells (t, s_begin[b, t] + s), 1 <= S <= 64; s_begin [B, T] integers (any value is
    legal), or k2's ranges [B, T, S], of which [..., 0] is taken; labels [B, L_max]; input_lengths / label_lengths [B].
    topology "standard" (the lattice of rnnt_loss) or "modified" (one symbol per frame).  fastemit_lambda in [0, 1] scales the
    gradient through the label edges by 1 + lambda; the costs do not depend on it.  A band that does not connect (0, 0) to the
    end costs +inf, with zero gradients.  Returns costs [B]: float32 on a device, float64 from the CPU mirror."""
    topology = check_topology(topology)
    lam = check_fastemit_lambda(fastemit_lambda)
    acts_c, sb, labels, il, ll, maxU = _inputs("rnnt_loss_pruned", acts, s_begin, labels, input_lengths, label_lengths)
    blank = _check_blank("rnnt_loss_pruned", blank_label, acts.shape[3])
    fn = _RNNTPrunedLossFunction if acts.is_cuda else _RNNTPrunedMirrorFunction
    return fn.apply(acts if acts.is_contiguous() else acts.contiguous(), sb, labels, il, ll, blank, lam, topology, maxU)


def rnnt_loss_pruned_and_grad(acts, s_begin, labels, input_lengths, label_lengths, blank_label: int = 0,
                              fastemit_lambda: float = 0.0, topology: str = "standard"):
    """compute_rnnt_loss_pruned as one combined call: (costs [B], grads [B, T, S, V]) with grads = d cost_b / d acts (unscaled).
    The arguments of rnnt_loss_pruned; no autograd graph is built.  CPU tensors: the float64 mirror (float64 results)."""
    topology = check_topology(topology)
    lam = check_fastemit_lambda(fastemit_lambda)
    acts_c, sb, labels, il, ll, maxU = _inputs("rnnt_loss_pruned_and_grad", acts, s_begin, labels, input_lengths, label_lengths)
    blank = _check_blank("rnnt_loss_pruned_and_grad", blank_label, acts.shape[3])
    if not acts_c.is_cuda:
        return _mirror(acts_c, sb, labels, il, ll, blank, lam, topology, maxU)
    B, T, S, V = acts_c.shape
    with torch.cuda.device(acts_c.device):
        ws = torch.empty(_lib.pruned_workspace_bytes(T, S, B), dtype=torch.uint8, device=acts_c.device)
        costs = torch.empty(B, dtype=torch.float32, device=acts_c.device)
        grads = torch.empty_like(acts_c)
    _pruned_call(acts_c, grads, sb, labels, il, ll, None, costs, ws, blank, lam, topology, maxU)
    return costs, grads


def _ordered_ranges_call(occupancy, input_lengths, label_lengths, S):
    """compute_rnnt_prune_ranges (include/rnnt_prune_ranges.h, libwarprnnt_pruneranges.so) on the current stream: s_begin [B, T] int32."""
    if occupancy.dtype != torch.float32:
        raise TypeError("prune_ranges: ordered=True takes float32 occupancies on a device")
    B, T, U = occupancy.shape
    if B < 1 or T < 1 or not 1 <= U <= 8192:
        raise ValueError(f"prune_ranges: occupancy must be [B >= 1, T >= 1, 1 <= U <= 8192], got {tuple(occupancy.shape)}")
    dev = occupancy.device
    occ = occupancy.detach().contiguous()
    il, ll = _as_i32(input_lengths, dev).reshape(B), _as_i32(label_lengths, dev).reshape(B)
    with torch.cuda.device(dev):
        sb = torch.empty((B, T), dtype=torch.int32, device=dev)
        opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, T, U)
        st = _lib.load_pruneranges().compute_rnnt_prune_ranges(occ.data_ptr(), il.data_ptr(), ll.data_ptr(), B, S, sb.data_ptr(), opts)
    _lib.check(st, "compute_rnnt_prune_ranges")
    return sb


def prune_ranges(occupancy, input_lengths, label_lengths, s_range: int, ordered: bool = False):
    """Where each frame's band of `s_range` symbols begins: int32 [B, T] from per-cell occupancies [B, T, U] (non-negative:
    e_b + e_l per lattice cell, from whatever first pass the caller has).  Torch only, unless `ordered` is set.

    Per utterance (T_b frames, L_b labels, hi = max(0, L_b + 1 - s_range)), for the frames t < T_b:
      1. sb[t] is the LOWEST s0 in [0, hi] that maximises sum(occupancy[b, t, s0 : s0 + s_range]);
      2. sb[0] = 0, then sb[T_b - 1] = hi;
      3. a running maximum forwards: the result is non-decreasing;
      4. backwards over t = T_b - 2 ... 1: sb[t] = max(sb[t], sb[t + 1] - (s_range - 1)), so consecutive bands overlap;
      5. the frames t >= T_b repeat sb[T_b - 1].
    This is the same idea as k2's get_rnnt_prune_ranges but NOT bit-compatible with it: the rule above is the definition.

    The window sum of step 1 is a float64 torch `sum`, whose order of additions torch chooses: on peaked occupancies (one entry
    near 1, its neighbours at 1e-11 ... 1e-20) two windows that both hold the peak differ by less than an ulp, and which of them
    wins depends on that order.  ordered=True fixes it (include/rnnt_prune_ranges.h): w(s0) = ((occ[s0] + occ[s0 + 1]) + ...) +
    occ[s0 + S - 1], the terms widened to float64 and added in increasing s; the lowest s0 wins by a strict > from -inf, so a NaN
    sum never wins.  Steps 2 - 5 are the same.  A device tensor (float32) then runs the HIP library (two launches, no temporaries;
    no eager fallback: a missing library is an error), a CPU tensor a torch mirror of the same rule: the same occupancies give
    the same band on every route.  ordered=False is the rule above as it always was."""
    if occupancy.dim() != 3:
        raise ValueError("prune_ranges: occupancy must be [B, T, U]")
    S = int(s_range)
    if not 1 <= S <= MAX_S_RANGE:
        raise ValueError(f"prune_ranges: s_range must be in 1 ... {MAX_S_RANGE}, got {s_range!r}")
    B, T, U = occupancy.shape
    dev = occupancy.device
    if input_lengths.numel() != B or label_lengths.numel() != B:
        raise ValueError("prune_ranges: input_lengths and label_lengths must be [B]")
    if ordered and occupancy.is_cuda:
        return _ordered_ranges_call(occupancy, input_lengths, label_lengths, S)
    Tb = input_lengths.to(device=dev, dtype=torch.int64).reshape(B).clamp(1, T)
    Lb = label_lengths.to(device=dev, dtype=torch.int64).reshape(B).clamp(0, U - 1)
    hi = (Lb + 1 - S).clamp(min=0)
    occ = torch.nn.functional.pad(occupancy.detach().to(torch.float64), (0, S - 1))
    s0 = torch.arange(U, device=dev)
    if ordered:  # the mirror of the ordered rule: the same left-to-right additions, vectorised over s0
        win = occ[..., 0:U]
        for s in range(1, S):
            win = win + occ[..., s:s + U]
        # a window beyond hi and a NaN sum never win; where nothing beats -inf the answer is 0 (the lowest s0 of the maximum)
        win = torch.where((s0[None, None, :] <= hi[:, None, None]) & ~torch.isnan(win), win, torch.full_like(win, _NEG_INF))
    else:
        win = occ.unfold(-1, S, 1).sum(-1)  # [B, T, U]: the window that starts at s0 (cut off at U)
        win = torch.where(s0[None, None, :] <= hi[:, None, None], win, torch.full_like(win, -1.0))
    best = win.max(dim=-1, keepdim=True).values
    sb = torch.where(win == best, s0[None, None, :], torch.full((1, 1, 1), U, device=dev, dtype=torch.int64)).min(dim=-1).values
    t = torch.arange(T, device=dev)[None, :]
    live = t < Tb[:, None]
    last = t == (Tb - 1)[:, None]
    sb = torch.where(live, sb, torch.zeros_like(sb))
    sb[:, 0] = 0
    sb = torch.where(last, hi[:, None], sb)
    sb = torch.cummax(sb, dim=1).values
    # step 4 in closed form: sb[t] = max over k in [t, T_b - 1] of sb[k] - (k - t)(S - 1), for 1 <= t <= T_b - 2
    w = torch.where(live, sb - t * (S - 1), torch.full_like(sb, -(1 << 40)))
    back = torch.cummax(w.flip(1), dim=1).values.flip(1) + t * (S - 1)
    sb = torch.where(live & (t >= 1), torch.maximum(sb, back), sb)
    sb = torch.where(live, sb, hi[:, None])
    return sb.to(torch.int32)


def prune_joint_inputs(enc, pred, s_begin, s_range: int):
    """The joint's inputs for the band: (enc[:, :, None, :], pred gathered to [B, T, S, J]) from enc [B, T, J], pred [B, U, J] and
    s_begin [B, T] (or [B, T, S], of which [..., 0] is taken).  Row (b, t, s) of the second is pred[b, clamp(s_begin[b, t] + s, 0, U - 1)]:
    a clamped row feeds an absent cell, whose logits the loss does not read.  Differentiable in both."""
    if enc.dim() != 3 or pred.dim() != 3 or enc.shape[0] != pred.shape[0]:
        raise ValueError("prune_joint_inputs: enc must be [B, T, J] and pred [B, U, J]")
    S = int(s_range)
    if not 1 <= S <= MAX_S_RANGE:
        raise ValueError(f"prune_joint_inputs: s_range must be in 1 ... {MAX_S_RANGE}, got {s_range!r}")
    B, T = enc.shape[:2]
    U, J = pred.shape[1:]
    if s_begin.dim() == 3:
        s_begin = s_begin[..., 0]
    if tuple(s_begin.shape) != (B, T):
        raise ValueError(f"prune_joint_inputs: s_begin must be [B, T] = [{B}, {T}], got {tuple(s_begin.shape)}")
    idx = s_begin.to(device=pred.device, dtype=torch.int64)[:, :, None] + torch.arange(S, device=pred.device)[None, None, :]
    idx = idx.clamp(0, U - 1)
    gathered = torch.gather(pred[:, None].expand(B, T, U, J), 2, idx[..., None].expand(B, T, S, J))
    return enc[:, :, None, :], gathered
