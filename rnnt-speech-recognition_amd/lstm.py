"""One LSTM layer for training on the engine (include/rnnt.h compute_rnnt_lstm_train_fwd / _bwd; csrc/lstm_train_kernels.hip).

`LSTMLayerFunction` is a one-layer, batch-first, zero-initial-state LSTM (torch's gate order i, f, g, o; an optional bias-free
projection W_hr, as nn.LSTM's proj_size) whose forward keeps the activated gates, every c_t (and h_t where projected) and whose
backward is back-propagation through time written out by hand:

    forward, t = 0 ... T-1     a_t = pre_t + r_{t-1} W_hh^T,  pre = x W_ih^T + b_ih + b_hh
                               i, f, o = sigma(a_i), sigma(a_f), sigma(a_o);  g = tanh(a_g)
                               c_t = f c_{t-1} + i g;  h_t = o tanh(c_t);  r_t = h_t W_hr^T (projected) or h_t
    backward, t = T-1 ... 0    dr_t = dy_t + da_{t+1} W_hh;  dh_t = dr_t W_hr (projected) or dr_t
                               dc_t = dh_t o (1 - tanh^2 c_t) + dc_{t+1} f_{t+1}
                               da_o = dh_t tanh(c_t) o (1 - o);  da_i = dc_t g i (1 - i)
                               da_f = dc_t c_{t-1} f (1 - f);    da_g = dc_t i (1 - g^2)
    then, over all frames at once:
                               dW_ih = da^T x;  dW_hh = da[1:]^T r[:-1];  db_ih = db_hh = sum da;  dx = da W_ih;  dW_hr = dr^T h

On a float32 CUDA tensor the two recurrences are the library's HIP step kernels (one launch per frame for an unprojected layer,
two for a projected one, in each direction); `pre` and the five products after the backward are large GEMMs and go through
torch.matmul.  On a CPU tensor the SAME equations run as a torch loop in the tensor's dtype, so the formulas are checked on a
machine without a GPU.  There is no other route: a CUDA tensor that is not float32 is an error.  Only y is returned; the final
state is not an output.  Double backward is not supported."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _lib

MAX_ROWS, MAX_WIDTH, MAX_FRAMES = 1024, 4096, 1 << 20

# test hook: byte written into every new workspace and output buffer before a call (tests/test_lstm_train_gpu.py)
_BUFFER_FILL = None


def _empty(shape, dev) -> torch.Tensor:
    t = torch.empty(shape, dtype=torch.float32, device=dev)
    if _BUFFER_FILL is not None:
        t.view(torch.uint8).fill_(int(_BUFFER_FILL))
    return t


def _workspace(R: int, T: int, H: int, P: int, dev) -> torch.Tensor:
    ws = torch.empty(_lib.lstm_train_workspace_bytes(R, T, H, P), dtype=torch.uint8, device=dev)
    if _BUFFER_FILL is not None:
        ws.fill_(int(_BUFFER_FILL))
    return ws


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _check_engine(gates: torch.Tensor, w_hh: torch.Tensor, w_hr: Optional[torch.Tensor]) -> Tuple[int, int, int, int]:
    if not gates.is_cuda:
        raise TypeError("the engine LSTM runs on CUDA tensors (CPU tensors take torch_forward / torch_backward)")
    T, R, G = gates.shape
    H, P = G // 4, w_hh.shape[1]
    for t in (gates, w_hh) + (() if w_hr is None else (w_hr,)):
        if t.dtype != torch.float32 or t.device != gates.device or not t.is_contiguous() or t.data_ptr() % 16:
            raise TypeError("the engine LSTM takes contiguous, 16-byte aligned float32 tensors on one device")
    if tuple(w_hh.shape) != (4 * H, P) or (w_hr is not None and tuple(w_hr.shape) != (P, H)) or (w_hr is None and P != H):
        raise ValueError(f"LSTM weight shapes do not fit: gates {tuple(gates.shape)}, W_hh {tuple(w_hh.shape)}")
    if not (1 <= R <= MAX_ROWS and 1 <= T <= MAX_FRAMES and 1 <= P <= H <= MAX_WIDTH):
        raise ValueError(f"the engine LSTM takes rows <= {MAX_ROWS}, frames <= {MAX_FRAMES} and widths <= {MAX_WIDTH}; "
                         f"got rows {R}, frames {T}, hidden {H}, proj {P}")
    return T, R, H, P


def engine_forward(pre: torch.Tensor, w_hh: torch.Tensor, w_hr: Optional[torch.Tensor]):
    """The forward recurrence on the GPU.  pre [T, R, 4H] (time-major, float32, contiguous) is OVERWRITTEN by the activated
    gates.  -> (y [T, R, P], c [T, R, H], h [T, R, H] or None for an unprojected layer)."""
    T, R, H, P = _check_engine(pre, w_hh, w_hr)
    dev = pre.device
    with torch.cuda.device(dev):
        y, c = _empty((T, R, P), dev), _empty((T, R, H), dev)
        h = None if w_hr is None else _empty((T, R, H), dev)
        ws = _workspace(R, T, H, P, dev)
        opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, 1, 1)
        st = _lib.load().compute_rnnt_lstm_train_fwd(pre.data_ptr(), w_hh.data_ptr(), _ptr(w_hr), y.data_ptr(), c.data_ptr(), _ptr(h),
                                                     R, T, H, P, ws.data_ptr(), opts)
    _lib.check(st, "compute_rnnt_lstm_train_fwd")
    return y, c, h


def engine_backward(gates: torch.Tensor, c: torch.Tensor, dy: torch.Tensor, w_hh: torch.Tensor, w_hr: Optional[torch.Tensor]):
    """The backward recurrence on the GPU.  gates [T, R, 4H] (the forward's) is OVERWRITTEN by da.
    -> dr [T, R, P] for a projected layer, None otherwise (dr = dh is not kept)."""
    T, R, H, P = _check_engine(gates, w_hh, w_hr)
    dev = gates.device
    for t, shape in ((c, (T, R, H)), (dy, (T, R, P))):
        if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or tuple(t.shape) != shape or t.data_ptr() % 16:
            raise TypeError("the engine LSTM takes contiguous float32 c [T, R, H] and dy [T, R, P] on the gates' device")
    with torch.cuda.device(dev):
        dr = None if w_hr is None else _empty((T, R, P), dev)
        ws = _workspace(R, T, H, P, dev)
        opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, 1, 1)
        st = _lib.load().compute_rnnt_lstm_train_bwd(gates.data_ptr(), c.data_ptr(), dy.data_ptr(), w_hh.data_ptr(), _ptr(w_hr),
                                                     _ptr(dr), R, T, H, P, ws.data_ptr(), opts)
    _lib.check(st, "compute_rnnt_lstm_train_bwd")
    return dr


def torch_forward(pre: torch.Tensor, w_hh: torch.Tensor, w_hr: Optional[torch.Tensor]):
    """The engine's forward equations as a torch loop in pre's dtype (same arguments and results as engine_forward)."""
    T, R, G = pre.shape
    H, P = G // 4, w_hh.shape[1]
    y, c = pre.new_empty(T, R, P), pre.new_empty(T, R, H)
    h = None if w_hr is None else pre.new_empty(T, R, H)
    r_prev, c_prev = pre.new_zeros(R, P), pre.new_zeros(R, H)
    for t in range(T):
        a = pre[t] + r_prev @ w_hh.t()
        i, f, g, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
        pre[t] = torch.cat([i, f, g, o], dim=1)
        c[t] = f * c_prev + i * g
        ht = o * torch.tanh(c[t])
        if w_hr is None:
            y[t] = ht
        else:
            h[t] = ht
            y[t] = ht @ w_hr.t()
        r_prev, c_prev = y[t], c[t]
    return y, c, h


def torch_backward(gates: torch.Tensor, c: torch.Tensor, dy: torch.Tensor, w_hh: torch.Tensor, w_hr: Optional[torch.Tensor]):
    """The engine's backward equations as a torch loop (same arguments and results as engine_backward)."""
    T, R, G = gates.shape
    H = G // 4
    dr_all = None if w_hr is None else dy.new_empty(dy.shape)
    carry = None  # dc_{t+1} f_{t+1}
    for t in range(T - 1, -1, -1):
        dr = dy[t] if t == T - 1 else dy[t] + gates[t + 1] @ w_hh
        if w_hr is None:
            dh = dr
        else:
            dr_all[t] = dr
            dh = dr @ w_hr
        i, f, g, o = gates[t, :, :H], gates[t, :, H:2 * H], gates[t, :, 2 * H:3 * H], gates[t, :, 3 * H:]
        tc = torch.tanh(c[t])
        dc = dh * o * (1 - tc * tc)
        if carry is not None:
            dc = dc + carry
        c_prev = c[t - 1] if t else torch.zeros_like(c[0])
        carry = dc * f
        gates[t] = torch.cat([dc * g * (i * (1 - i)), dc * c_prev * (f * (1 - f)), dc * i * (1 - g * g), dh * tc * (o * (1 - o))], dim=1)
    return dr_all


class LSTMLayerFunction(torch.autograd.Function):
    """y = LSTMLayerFunction.apply(x, w_ih, w_hh, b_ih, b_hh, w_hr): x [B, T, I] batch-first, the weights as nn.LSTM holds them
    (w_ih [4H, I], w_hh [4H, P], b_ih, b_hh [4H], w_hr [P, H] or None) -> y [B, T, P]."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, w_hr=None):
        if x.dim() != 3:
            raise ValueError(f"x must be [batch, frames, features], got {tuple(x.shape)}")
        engine = x.is_cuda
        if engine and any(t.dtype != torch.float32 for t in (x, w_ih, w_hh, b_ih, b_hh) + (() if w_hr is None else (w_hr,))):
            raise TypeError('the engine LSTM is float32 only; use lstm="torch" for other types on the GPU')
        B, T, I = x.shape
        xt = x.detach().transpose(0, 1).contiguous()  # time-major: a frame's rows contiguous
        w_ih_, w_hh_ = w_ih.detach().contiguous(), w_hh.detach().contiguous()
        w_hr_ = None if w_hr is None else w_hr.detach().contiguous()
        pre = torch.addmm(b_ih.detach() + b_hh.detach(), xt.reshape(T * B, I), w_ih_.t()).view(T, B, -1)
        y, c, h = (engine_forward if engine else torch_forward)(pre, w_hh_, w_hr_)
        ctx.engine = engine
        ctx.save_for_backward(xt, w_ih_, w_hh_, w_hr_, pre, c, h, y)  # pre now holds the activated gates
        return y.transpose(0, 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        xt, w_ih, w_hh, w_hr, gates, c, h, y = ctx.saved_tensors
        T, B, I = xt.shape
        G, P = gates.shape[2], y.shape[2]
        dyt = dy.transpose(0, 1).contiguous()
        da = gates.clone()  # the saved gates stay intact: backward may be called again with retain_graph
        dr = (engine_backward if ctx.engine else torch_backward)(da, c, dyt, w_hh, w_hr)
        need = ctx.needs_input_grad
        da2 = da.view(T * B, G)
        dx = (da2 @ w_ih).view(T, B, I).transpose(0, 1) if need[0] else None
        dw_ih = da2.t() @ xt.reshape(T * B, I) if need[1] else None
        dw_hh = None
        if need[2]:
            dw_hh = da[1:].reshape((T - 1) * B, G).t() @ y[:-1].reshape((T - 1) * B, P) if T > 1 else torch.zeros_like(w_hh)
        db = da2.sum(0) if (need[3] or need[4]) else None
        dw_hr = None
        if w_hr is not None and need[5]:
            dw_hr = dr.reshape(T * B, P).t() @ h.reshape(T * B, -1)
        return dx, dw_ih, dw_hh, db if need[3] else None, db if need[4] else None, dw_hr


def lstm_layer(lstm: torch.nn.LSTM, x: torch.Tensor) -> torch.Tensor:
    """forward of a one-layer, batch-first, unidirectional nn.LSTM (the parameter holder) through LSTMLayerFunction -> y."""
    if lstm.num_layers != 1 or lstm.bidirectional or not lstm.batch_first or not lstm.bias:
        raise ValueError('lstm="engine" takes a one-layer, unidirectional, batch-first nn.LSTM with biases')
    w_hr = lstm.weight_hr_l0 if lstm.proj_size else None
    return LSTMLayerFunction.apply(x, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, w_hr)
