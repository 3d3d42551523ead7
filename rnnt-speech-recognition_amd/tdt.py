"""The token-and-duration (TDT) transducer loss (include/rnnt_tdt.h compute_rnnt_loss_tdt, libwarprnnt_tdt.so) and a greedy TDT
decoder.

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
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
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
    one frame with d == 0.  Then t += d, until t >= T (the last jump may pass T)."""
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
