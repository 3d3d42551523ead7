"""Joint network fused with the transducer loss (host side).

Reference: model.py:158-166 (broadcast add -> Dense(J, tanh) -> Dense(V)) followed by
utils/loss.py:24-36 and TF autodiff (run_rnnt.py:284).  The first Dense layer is applied to the
encoder and prediction-network outputs separately (exact factorisation) and the whole network runs
behind the C ABI: libwarprnnt.so's compute_rnnt_joint_net_loss_* entry points do the two W1 GEMMs and
their backward (csrc/dense_kernels.hip), tanh, the J x V projection on the MFMA units, log-softmax,
alpha/beta, and the gradient scatter back to enc / pred / W1 / b1 / W2 / b2, without ever materialising
[B,T,U,J] or [B,T,U,V] tensors.  Hidden sizes the dense kernels do not take (not a multiple of 32) go
through torch.matmul + autograd around compute_rnnt_joint_loss_* (first_layer="torch").
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._lib import ptr


class _JointLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc_proj, pred_proj, W2, b2, labels, input_lengths, label_lengths, blank_label, joint_dtype, fastemit_lambda=0.0):
        lib = _lib.load()
        for name, x in (("enc_proj", enc_proj), ("pred_proj", pred_proj), ("W2", W2), ("b2", b2)):
            if not x.is_cuda:
                raise RuntimeError(f"rnnt_joint_loss: {name} must live on an MI355X (cuda/HIP) device; no CPU path")
            if x.dtype != torch.float32:
                raise TypeError(f"rnnt_joint_loss: {name} must be float32")
        B, T, J = enc_proj.shape
        U = pred_proj.shape[1]
        V = W2.shape[1]
        if pred_proj.shape != (B, U, J) or W2.shape[0] != J or b2.shape != (V,):
            raise ValueError("rnnt_joint_loss: inconsistent shapes")
        dev = enc_proj.device
        ep, pp, w2, bb = (x.detach().contiguous() for x in (enc_proj, pred_proj, W2, b2))
        labels = labels.to(device=dev, dtype=torch.int32).contiguous()
        # the kernels index labels with row stride U-1: any other width would silently read the wrong labels
        if U > 1 and tuple(labels.shape) != (B, U - 1):
            raise ValueError(f"rnnt_joint_loss: labels must be [B, U-1] = [{B}, {U - 1}], got {tuple(labels.shape)}")
        if labels.numel() == 0:
            labels = torch.zeros((B, 1), dtype=torch.int32, device=dev)
        il = input_lengths.to(device=dev, dtype=torch.int32).contiguous()
        ll = label_lengths.to(device=dev, dtype=torch.int32).contiguous()
        if il.numel() != B or ll.numel() != B:
            raise ValueError("rnnt_joint_loss: input_lengths and label_lengths must be [B]")
        with torch.cuda.device(dev):
            ws = _new_workspace(_lib.joint_workspace_bytes(T, U, B, J, V), dev)
            costs = torch.empty(B, dtype=torch.float32, device=dev)
            opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, int(blank_label), T, U)
            if any(ctx.needs_input_grad[:4]):
                # _fwd = "a _bwd call on this workspace follows": the f16 joint parks its softmax numerators for it
                st = lib.compute_rnnt_joint_loss_fwd(ep.data_ptr(), pp.data_ptr(), w2.data_ptr(), bb.data_ptr(),
                                                     labels.data_ptr(), ll.data_ptr(), il.data_ptr(), J, V, B,
                                                     costs.data_ptr(), int(joint_dtype), ws.data_ptr(), opts)
            else:  # costs only (evaluation)
                st = lib.compute_rnnt_joint_loss(ep.data_ptr(), pp.data_ptr(), w2.data_ptr(), bb.data_ptr(),
                                                 labels.data_ptr(), ll.data_ptr(), il.data_ptr(), None, J, V, B,
                                                 costs.data_ptr(), None, None, None, None, int(joint_dtype), ws.data_ptr(), opts)
        _lib.check(st, "compute_rnnt_joint_loss_fwd")
        ctx.save_for_backward(ep, pp, w2, bb, labels, il, ll, ws)
        ctx.blank = int(blank_label)
        ctx.joint_dtype = int(joint_dtype)
        ctx.fastemit_lambda = float(fastemit_lambda)
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        ep, pp, w2, bb, labels, il, ll, ws = ctx.saved_tensors
        lib = _lib.load()
        B, T, J = ep.shape
        U, V = pp.shape[1], w2.shape[1]
        dev = ep.device
        scale = grad_costs.to(device=dev, dtype=torch.float32).contiguous()
        with torch.cuda.device(dev):
            d_ep, d_pp, d_w2, d_b2 = (torch.empty_like(x) for x in (ep, pp, w2, bb))
            opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, ctx.blank, T, U)
            args = (ep.data_ptr(), pp.data_ptr(), w2.data_ptr(), bb.data_ptr(),
                    labels.data_ptr(), ll.data_ptr(), il.data_ptr(), scale.data_ptr(),
                    J, V, B, d_ep.data_ptr(), d_pp.data_ptr(), d_w2.data_ptr(),
                    d_b2.data_ptr(), ctx.joint_dtype, ws.data_ptr(), opts)
            if ctx.fastemit_lambda != 0.0:
                st = lib.compute_rnnt_joint_loss_bwd_fastemit(*args, ctx.fastemit_lambda)
            else:
                st = lib.compute_rnnt_joint_loss_bwd(*args)
            _lib.check(st, "compute_rnnt_joint_loss_bwd")
            _note_backward_rows(ws, T, U, B, J, V, ctx.blank)
        return d_ep, d_pp, d_w2, d_b2, None, None, None, None, None, None


class _JointNetLossFunction(torch.autograd.Function):
    """The whole joint network + loss behind the C ABI (compute_rnnt_joint_net_loss_fwd / _bwd): the first Dense layer and its
    backward run in the library too (csrc/dense_kernels.hip), not in torch."""

    @staticmethod
    def forward(ctx, enc, pred, W1, b1, W2, b2, labels, input_lengths, label_lengths, blank_label, joint_dtype, fastemit_lambda=0.0):
        lib = _lib.load()
        for name, x in (("enc", enc), ("pred", pred), ("W1", W1), ("b1", b1), ("W2", W2), ("b2", b2)):
            if not x.is_cuda:
                raise RuntimeError(f"rnnt_joint_loss: {name} must live on an MI355X (cuda/HIP) device; no CPU path")
            if x.dtype != torch.float32:
                raise TypeError(f"rnnt_joint_loss: {name} must be float32")
        B, T, H = enc.shape
        U = pred.shape[1]
        J, V = W2.shape
        if pred.shape != (B, U, H) or W1.shape != (H, J) or b1.shape != (J,) or b2.shape != (V,):
            raise ValueError("rnnt_joint_loss: inconsistent shapes")
        dev = enc.device
        e, p, w1, bb1, w2, bb2 = (x.detach().contiguous() for x in (enc, pred, W1, b1, W2, b2))
        # the dense kernels move 16 bytes per access: an operand that is contiguous but starts off that grid (a slice of a flat
        # parameter bucket, say) is copied to a fresh allocation instead of being refused
        e, p, w1, bb1 = (x if x.data_ptr() % 16 == 0 else x.clone() for x in (e, p, w1, bb1))
        labels = labels.to(device=dev, dtype=torch.int32).contiguous()
        if U > 1 and tuple(labels.shape) != (B, U - 1):
            raise ValueError(f"rnnt_joint_loss: labels must be [B, U-1] = [{B}, {U - 1}], got {tuple(labels.shape)}")
        if labels.numel() == 0:
            labels = torch.zeros((B, 1), dtype=torch.int32, device=dev)
        il = input_lengths.to(device=dev, dtype=torch.int32).contiguous()
        ll = label_lengths.to(device=dev, dtype=torch.int32).contiguous()
        if il.numel() != B or ll.numel() != B:
            raise ValueError("rnnt_joint_loss: input_lengths and label_lengths must be [B]")
        with torch.cuda.device(dev):
            ws = _new_workspace(_lib.joint_net_workspace_bytes(T, U, B, H, J, V), dev)
            costs = torch.empty(B, dtype=torch.float32, device=dev)
            opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, int(blank_label), T, U)
            if any(ctx.needs_input_grad[:6]):
                st = lib.compute_rnnt_joint_net_loss_fwd(e.data_ptr(), p.data_ptr(), w1.data_ptr(), bb1.data_ptr(), w2.data_ptr(),
                                                         bb2.data_ptr(), labels.data_ptr(), ll.data_ptr(), il.data_ptr(), H, J, V, B,
                                                         costs.data_ptr(), int(joint_dtype), ws.data_ptr(), opts)
            else:  # costs only (evaluation)
                st = lib.compute_rnnt_joint_net_loss(e.data_ptr(), p.data_ptr(), w1.data_ptr(), bb1.data_ptr(), w2.data_ptr(),
                                                     bb2.data_ptr(), labels.data_ptr(), ll.data_ptr(), il.data_ptr(), None, H, J, V, B,
                                                     costs.data_ptr(), None, None, None, None, None, None, int(joint_dtype),
                                                     ws.data_ptr(), opts)
        _lib.check(st, "compute_rnnt_joint_net_loss_fwd")
        ctx.save_for_backward(e, p, w1, bb1, w2, bb2, labels, il, ll, ws)
        ctx.blank = int(blank_label)
        ctx.joint_dtype = int(joint_dtype)
        ctx.fastemit_lambda = float(fastemit_lambda)
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        e, p, w1, bb1, w2, bb2, labels, il, ll, ws = ctx.saved_tensors
        lib = _lib.load()
        B, T, H = e.shape
        U = p.shape[1]
        J, V = w2.shape
        dev = e.device
        scale = grad_costs.to(device=dev, dtype=torch.float32).contiguous()
        with torch.cuda.device(dev):
            grads = [torch.empty_like(x) for x in (e, p, w1, bb1, w2, bb2)]
            opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, ctx.blank, T, U)
            args = (e.data_ptr(), p.data_ptr(), w1.data_ptr(), bb1.data_ptr(), w2.data_ptr(),
                    bb2.data_ptr(), labels.data_ptr(), ll.data_ptr(), il.data_ptr(),
                    scale.data_ptr(), H, J, V, B, *(g.data_ptr() for g in grads),
                    ctx.joint_dtype, ws.data_ptr(), opts)
            if ctx.fastemit_lambda != 0.0:
                st = lib.compute_rnnt_joint_net_loss_bwd_fastemit(*args, ctx.fastemit_lambda)
            else:
                st = lib.compute_rnnt_joint_net_loss_bwd(*args)
            _lib.check(st, "compute_rnnt_joint_net_loss_bwd")
            _note_backward_rows(ws, T, U, B, J, V, ctx.blank)
        return (*grads, None, None, None, None, None, None)


JOINT_DTYPES = {"f32": 0, "f16": 1}

# Diagnostics (off by default): with TRACK_BACKWARD_ROWS set, every backward of this module asks the library how many lattice rows
# (x 32-column tiles) it visited -- the data-dependent part of the f32-grade joint's run time (include/rnnt.h
# get_rnnt_joint_backward_rows; the query synchronises the stream) -- and last_backward_rows() returns the answer.
TRACK_BACKWARD_ROWS = False
_LAST_ROWS = None


def _note_backward_rows(ws, T, U, B, J, V, blank):
    global _LAST_ROWS
    if not TRACK_BACKWARD_ROWS:
        return
    import ctypes

    rows = (ctypes.c_int * 2)(-1, -1)
    opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, blank, T, U)
    st = _lib.load().get_rnnt_joint_backward_rows(ws.data_ptr(), J, V, B, opts, rows)
    _LAST_ROWS = (rows[0], rows[1]) if st == 0 else (-1, -1)


def last_backward_rows():
    """(rows x 32-column tiles the last tracked backward visited, rows inside the utterances); (-1, -1) where nothing is skipped
    (the f16 joint, the wide joint); None when nothing was tracked (TRACK_BACKWARD_ROWS)."""
    return _LAST_ROWS


# Test hook: when set to a byte value, every workspace this module allocates is filled with it before the forward call
# (0xFF = a NaN bit pattern in every float: a backward kernel that read a workspace word nobody wrote would show it).
_WORKSPACE_FILL = None


def _new_workspace(nbytes: int, dev) -> torch.Tensor:
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if _WORKSPACE_FILL is not None:
        ws.fill_(int(_WORKSPACE_FILL))
    return ws


def _workspace(ws, nbytes: int, dev) -> torch.Tensor:
    """The workspace an object that owns one begins on: `ws`, the one it has, when that lives on dev and holds nbytes (filled
    again under the test hook), else a fresh one."""
    if ws is None or ws.device != dev or ws.numel() < nbytes:
        return _new_workspace(nbytes, dev)
    if _WORKSPACE_FILL is not None:
        ws.fill_(int(_WORKSPACE_FILL))
    return ws


def rnnt_joint_loss(enc, pred, W1, b1, W2, b2, labels, input_lengths, label_lengths, blank_label: int = 0,
                    joint_dtype: str = "auto", first_layer: str = "auto", visit_all: bool = False,
                    fastemit_lambda: float = 0.0):
    """costs[b] = transducer NLL of  logits = tanh((enc[:,:,None]+pred[:,None]) @ W1 + b1) @ W2 + b2.

    enc [B,T,H] (encoder output), pred [B,U,H] (prediction-network output), W1 [H,J], b1 [J],
    W2 [J,V], b2 [V]  (Keras Dense kernels are stored [in, out], model.py:162-166).

    joint_dtype: arithmetic of the J x V product.  "f32": f32-grade products (binary16 hi + lo operands on the f16 MFMA units, f32 accumulation), small vocabularies (V <= 32, the reference's
    character set; up to 128 symbols at joint sizes up to 640, as up to four vocabulary tiles -- "auto" uses it up to 64).  "f16": operands rounded to binary16, f32 accumulation, for large vocabularies -- the counterpart
    of the reference's `mixed_float16` policy (run_rnnt.py:96-99); the lattice stays f32 either way.  "auto" picks by V.
    Shapes the kernels do not take natively (f16: V a multiple of 128, J a multiple of 128 up to 640; f32: J a multiple of
    64) are padded up exactly (zero units / zero-probability symbols).

    first_layer: where the first Dense layer (enc @ W1 + b1, pred @ W1, and dW1 / db1 / d enc / d pred) runs.  "engine": inside
    libwarprnnt.so (compute_rnnt_joint_net_loss_*: split-precision MFMA GEMMs, csrc/dense_kernels.hip; hidden size a multiple
    of 32).  "torch": torch.matmul + autograd around compute_rnnt_joint_loss_*.  "auto": the engine whenever it takes the shape.

    visit_all: RNNT_VISIT_ALL of include/rnnt.h -- the backward visits every lattice row instead of skipping the rows (x 32-column
    tiles) whose cells all have an occupancy below 2^-40 (their binary16 dlogits parts are exact zeros already: same results up to the
    order of a few f32 sums; timing then does not depend on the data).

    fastemit_lambda in [0, 1]: FastEmit regularisation (include/rnnt.h compute_rnnt_loss_fastemit) -- the backward starts from the
    dlogits with the label edges' gradient scaled by 1 + fastemit_lambda; the costs do not change."""
    from .loss import check_fastemit_lambda

    fastemit_lambda = check_fastemit_lambda(fastemit_lambda)
    dtype_word = lambda name: JOINT_DTYPES[name] | (_lib.RNNT_VISIT_ALL if visit_all else 0)  # noqa: E731
    if joint_dtype == "auto":
        joint_dtype = _auto_joint_dtype(W2.shape[0], W2.shape[1])
    if joint_dtype not in JOINT_DTYPES:
        raise ValueError(f"rnnt_joint_loss: joint_dtype must be one of {sorted(JOINT_DTYPES)} or 'auto'")
    # The kernels take a fixed set of (J, V) shapes; anything else is padded up here, exactly:
    #   joint units  -- extra units get zero W1 columns / b1 entries (projections 0) and zero W2 rows: h = tanh(0) = 0 contributes nothing;
    #   vocabulary   -- extra columns get zero weights and a bias of -1e4: their softmax mass is exp(-1e4) = 0 in f32.
    # Autograd slices the gradients back through the pads.
    J, V = W2.shape
    H = W1.shape[0]
    Jp, Vp = padded_joint_shape(J, V, joint_dtype)
    if Jp != J:
        W1 = torch.nn.functional.pad(W1, (0, Jp - J))
        b1 = torch.nn.functional.pad(b1, (0, Jp - J))
        W2 = torch.nn.functional.pad(W2, (0, 0, 0, Jp - J))
    if Vp != V:
        W2 = torch.nn.functional.pad(W2, (0, Vp - V))
        b2 = torch.nn.functional.pad(b2, (0, Vp - V), value=_PAD_BIAS)
    if first_layer == "auto":
        first_layer = "engine" if (H % 32 == 0 and Jp % 64 == 0 and max(H, Jp) <= 4096) else "torch"
    if first_layer == "engine":
        # the whole joint network behind the C ABI: W1 GEMMs, their backward, tanh, W2, the lattice (include/rnnt.h)
        return _JointNetLossFunction.apply(enc, pred, W1, b1, W2, b2, labels, input_lengths, label_lengths, blank_label,
                                           dtype_word(joint_dtype), fastemit_lambda)
    if first_layer != "torch":
        raise ValueError("rnnt_joint_loss: first_layer must be 'auto', 'engine' or 'torch'")
    # hidden sizes the library's dense kernels do not take (not a multiple of 32): the first layer through torch.matmul
    # (hipBLASLt) and autograd, the rest through compute_rnnt_joint_loss
    enc_proj = torch.matmul(enc, W1) + b1
    pred_proj = torch.matmul(pred, W1)
    return _JointLossFunction.apply(enc_proj, pred_proj, W2, b2, labels, input_lengths, label_lengths, blank_label,
                                    dtype_word(joint_dtype), fastemit_lambda)


_LOGITS_CACHE = {}  # (device, entry, shape) -> (workspace, output): a greedy decoder asks for one cell per emitted symbol


@torch.no_grad()
def joint_logits(enc, pred, W1, b1, W2, b2, joint_dtype: str = "auto", reuse_buffers: bool = False):
    """logits [B, T, U, V] of the joint network through libwarprnnt.so (no autograd): the decoding twin of the joint
    (utils/decoding.py:6-18).  Same factorisation, tables and products as the fused loss of the same joint_dtype ("f32": V <= 32,
    f32-grade; "f16": binary16 operands, up to 8192 symbols -- the reference's default 4096 word pieces; "auto" picks by V), so a
    decoder sees the logits the loss was trained on.  The first Dense layer runs in the library too (compute_rnnt_joint_net_logits)
    when the hidden size is a multiple of 32, else through torch.matmul in front of compute_rnnt_joint_logits.  Joint sizes /
    vocabularies the kernels do not take natively are padded exactly as in rnnt_joint_loss.

    reuse_buffers=True returns a VIEW OF A CACHED BUFFER (one workspace + output pair per device, stream and shape, at most
    eight pairs): the next call with the same shape on the same stream overwrites it.  Only for callers that consume the result
    before they call again (the greedy decoder asks for one lattice cell per emitted symbol); the default allocates."""
    lib = _lib.load()
    for name, x in (("enc", enc), ("pred", pred), ("W1", W1), ("W2", W2)):
        if not x.is_cuda:
            raise RuntimeError(f"joint_logits: {name} must live on an MI355X (cuda/HIP) device; no CPU path")
    B, T, H = enc.shape
    U = pred.shape[1]
    J, V = W2.shape
    if joint_dtype == "auto":
        joint_dtype = _auto_joint_dtype(J, V)
    Jp, Vp = padded_joint_shape(J, V, joint_dtype)
    if Jp != J:
        W1 = torch.nn.functional.pad(W1, (0, Jp - J))
        b1 = torch.nn.functional.pad(b1, (0, Jp - J))
        W2 = torch.nn.functional.pad(W2, (0, 0, 0, Jp - J))
    if Vp != V:
        W2 = torch.nn.functional.pad(W2, (0, Vp - V))
        b2 = torch.nn.functional.pad(b2, (0, Vp - V), value=_PAD_BIAS)
    dev = enc.device
    engine_first_layer = H % 32 == 0 and max(H, Jp) <= 4096
    with torch.cuda.device(dev):
        key = (dev, torch.cuda.current_stream().cuda_stream, engine_first_layer, T, U, B, H, Jp, Vp)
        if reuse_buffers and key in _LOGITS_CACHE:
            ws, out = _LOGITS_CACHE[key]
        else:
            nbytes = (_lib.joint_net_workspace_bytes(T, U, B, H, Jp, Vp) if engine_first_layer
                      else _lib.joint_workspace_bytes(T, U, B, Jp, Vp))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            out = torch.empty(B, T, U, Vp, dtype=torch.float32, device=dev)
            if reuse_buffers:  # (the caller consumes `out` before the next call: decoding.greedy_decode_fn does)
                if len(_LOGITS_CACHE) > 8:
                    _LOGITS_CACHE.clear()
                _LOGITS_CACHE[key] = (ws, out)
        opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, T, U)
        w2, bb = W2.detach().contiguous().float(), b2.detach().contiguous().float()
        if engine_first_layer:
            e, p, w1, bb1 = (x.detach().contiguous().float() for x in (enc, pred, W1, b1))
            e, p, w1, bb1 = (x if x.data_ptr() % 16 == 0 else x.clone() for x in (e, p, w1, bb1))
            st = lib.compute_rnnt_joint_net_logits(e.data_ptr(), p.data_ptr(), w1.data_ptr(), bb1.data_ptr(), w2.data_ptr(),
                                                   bb.data_ptr(), H, Jp, Vp, B, out.data_ptr(), JOINT_DTYPES[joint_dtype],
                                                   ws.data_ptr(), opts)
            _lib.check(st, "compute_rnnt_joint_net_logits")
        else:
            ep = (torch.matmul(enc.float(), W1) + b1).contiguous()
            pp = torch.matmul(pred.float(), W1).contiguous()
            st = lib.compute_rnnt_joint_logits(ep.data_ptr(), pp.data_ptr(), w2.data_ptr(), bb.data_ptr(), Jp, Vp, B,
                                               out.data_ptr(), JOINT_DTYPES[joint_dtype], ws.data_ptr(), opts)
            _lib.check(st, "compute_rnnt_joint_logits")
    return out if Vp == V else out[..., :V]


_PAD_BIAS = -1.0e4
_F16_J = (128, 256, 384, 512, 640)


def _auto_joint_dtype(J: int, V: int) -> str:
    """f32-grade products up to 64 symbols (32 at joint sizes above 640): one or two vocabulary tiles of the split-precision joint,
    as fast as the f16 joint on its smallest (128-column) shape and f32-grade; the f16 MFMA joint beyond.  (joint_dtype="f32"
    takes up to 128 symbols -- four tiles, four passes -- when f32-grade gradients matter more than time.)"""
    return "f32" if (V <= 32 or (V <= 64 and J <= 640)) else "f16"



def padded_joint_shape(J: int, V: int, joint_dtype: str):
    """(J, V) -> the nearest shape the chosen kernels accept (include/rnnt.h), or raises if there is none."""
    if joint_dtype == "f32":
        Jp = (J + 63) // 64 * 64
        if Jp > 704:
            raise ValueError("rnnt_joint_loss: the f32 joint takes joint sizes of at most 704")
        if V > (128 if Jp <= 640 else 32):
            raise ValueError("rnnt_joint_loss: the f32 joint takes vocabularies of at most 128 symbols (32 at joint sizes above 640); "
                             "use joint_dtype='f16'")
        return Jp, V
    Jp = next((j for j in _F16_J if j >= J), None)
    if Jp is None:
        raise ValueError("rnnt_joint_loss: the f16 joint takes joint sizes of at most 640")
    Vp = max(128, (V + 127) // 128 * 128)
    if Vp > 8192:
        raise ValueError("rnnt_joint_loss: the f16 joint takes vocabularies of at most 8192 symbols")
    return Jp, Vp


class JointLoss(torch.nn.Module):
    """The reference's joint network (model.py:158-166) + loss as one module.  Parameters follow Keras'
    Dense defaults: glorot-uniform kernels, zero biases."""

    def __init__(self, hidden: int, joint_size: int, vocab_size: int, blank_label: int = 0, visit_all: bool = False,
                 fastemit_lambda: float = 0.0):
        super().__init__()
        from .loss import check_fastemit_lambda

        self.blank_label = blank_label
        self.fastemit_lambda = check_fastemit_lambda(fastemit_lambda)  # FastEmit's weight on the label edges' gradient (rnnt_joint_loss)
        self.visit_all = visit_all  # RNNT_VISIT_ALL: no occupancy floor in the backward (rnnt_joint_loss)
        self.W1 = torch.nn.Parameter(torch.empty(hidden, joint_size))
        self.b1 = torch.nn.Parameter(torch.zeros(joint_size))
        self.W2 = torch.nn.Parameter(torch.empty(joint_size, vocab_size))
        self.b2 = torch.nn.Parameter(torch.zeros(vocab_size))
        for w in (self.W1, self.W2):
            lim = math.sqrt(6.0 / (w.shape[0] + w.shape[1]))
            torch.nn.init.uniform_(w, -lim, lim)

    def forward(self, enc, pred, labels, input_lengths, label_lengths):
        return rnnt_joint_loss(enc, pred, self.W1, self.b1, self.W2, self.b2, labels, input_lengths,
                               label_lengths, self.blank_label, visit_all=self.visit_all,
                               fastemit_lambda=self.fastemit_lambda)

    def logits(self, enc, pred):
        """Unfused reference form (materialises [B,T,U,J] and [B,T,U,V] in torch); for tests and host-logic checks on CPU."""
        z = enc.unsqueeze(2) + pred.unsqueeze(1)
        return torch.tanh(z @ self.W1 + self.b1) @ self.W2 + self.b2

    def cell_logits(self, enc, pred, reuse_buffers: bool = False):
        """Joint logits [B, T, U, V] for decoding (utils/decoding.py:6-18).  On an MI355X this is the ENGINE at every vocabulary
        size (compute_rnnt_joint_net_logits / compute_rnnt_joint_logits: the fused loss's own forward kernels, first Dense layer
        included); CPU tensors -- the host-logic tests -- and shapes the kernels do not take (joint sizes beyond 704 / 640) use
        the torch composition.  The result is a fresh tensor unless `reuse_buffers` is set (see joint_logits: the buffer is then
        overwritten by the next call of the same shape -- the greedy decoder opts in, a beam search must not)."""
        if enc.is_cuda:
            try:
                padded_joint_shape(self.W2.shape[0], self.W2.shape[1], _auto_joint_dtype(*self.W2.shape))
            except ValueError:
                return self.logits(enc, pred)
            return joint_logits(enc, pred, self.W1, self.b1, self.W2, self.b2, reuse_buffers=reuse_buffers)
        return self.logits(enc, pred)


def _projected_operand(pred_proj, Jp: int):
    if pred_proj.dtype != torch.float32 or pred_proj.dim() != 2 or pred_proj.shape[1] != Jp:
        raise ValueError(f"pred_proj must be float32 [rows, {Jp}] (the joint-unit padded pred @ W1)")
    return pred_proj.contiguous()


def _torch_cell_logits(joint: "JointLoss", e, pred, pred_proj):
    """One joint cell per row on the torch route: e [R, H] against pred [R, H] (JointLoss.logits), or against pred_proj
    [R, >= J] = pred @ W1 already (its first J columns): tanh(e W1 + b1 + pred_proj) W2 + b2 -> [R, V]."""
    if pred_proj is None:
        return joint.logits(e[:, None, :], pred[:, None, :])[:, 0, 0, :]
    J = joint.W1.shape[1]
    z = e @ joint.W1 + joint.b1 + pred_proj[:, :J].to(e.dtype)
    return torch.tanh(z) @ joint.W2 + joint.b2


class _EngineJoint:
    """What the decoder joints share: the engine / torch decision and the engine's weights.  `engine`: the joint's tensors are
    on a device and its shape is one the kernels take (the rule of JointLoss.cell_logits); then `dtype`, `Jp` and W1 / b1 / W2 / b2
    as float32 with the joint units zero-padded to Jp (as joint_logits pads them; the output columns need none: the step kernels
    skip padding columns themselves).  `V`: W2's columns (a TDT joint takes its duration head off them).  `_ws`: the workspace
    the object owns, kept by _workspace from one begin to the next."""

    def __init__(self, joint, joint_dtype: str = "auto", token_times: bool = False):
        self.joint = joint
        self.token_times = bool(token_times)
        self.blank = int(joint.blank_label)
        W1, b1, W2, b2 = (x.detach() for x in (joint.W1, joint.b1, joint.W2, joint.b2))
        J, self.V = W2.shape
        self.engine = W2.is_cuda
        if self.engine:
            if joint_dtype == "auto":
                joint_dtype = _auto_joint_dtype(J, self.V)
            try:
                Jp, _ = padded_joint_shape(J, self.V, joint_dtype)
            except ValueError:
                self.engine = False
        if self.engine:
            self.dtype = JOINT_DTYPES[joint_dtype]
            self.Jp = Jp
            pad = lambda x, p: torch.nn.functional.pad(x.float(), p).contiguous()  # noqa: E731
            self.W1, self.b1 = pad(W1, (0, Jp - J)), pad(b1, (0, Jp - J))
            self.W2, self.b2 = pad(W2, (0, 0, 0, Jp - J)), b2.float().contiguous()
        self._ws = None


class _GreedyEngineJoint(_EngineJoint):
    """What the greedy joints share beyond _EngineJoint: the output buffers (`hyps`, `lengths`, `emitted`, `all_done`, `scores`;
    `frames` and `logp`, None without token_times), grow_hyps, and the torch mirror's cursors."""

    def __init__(self, joint, joint_dtype: str = "auto", token_times: bool = False):
        super().__init__(joint, joint_dtype, token_times)
        self._frame_base = None  # (the stream: frames of the chunks a slot has left behind)

    def _new_outputs(self, rows: int, max_hyp_len: int, dev, all_done: int, torch_dtype):
        """scores: float32 on the engine, on the torch route torch_dtype where that is wider."""
        self.hyps = torch.zeros(rows, max_hyp_len, dtype=torch.int32, device=dev)
        self.lengths = torch.zeros(rows, dtype=torch.int32, device=dev)
        self.emitted = torch.full((rows,), -1, dtype=torch.int32, device=dev)
        self.all_done = torch.full((1,), all_done, dtype=torch.int32, device=dev)
        sdtype = torch.float32 if self.engine else torch.promote_types(torch_dtype, torch.float32)
        self.scores = torch.zeros(rows, dtype=sdtype, device=dev)
        self.frames = self.logp = None
        if self.token_times:
            self.frames = torch.full((rows, max_hyp_len), -1, dtype=torch.int32, device=dev)
            self.logp = torch.zeros(rows, max_hyp_len, dtype=sdtype, device=dev)

    def grow_hyps(self):
        """Double the hyps buffer (contents kept; `frames` and `logp` with it): paused hypotheses resume at the next step."""
        h = self.hyps
        self.hyps = torch.zeros(h.shape[0], 2 * h.shape[1], dtype=h.dtype, device=h.device)
        self.hyps[:, : h.shape[1]] = h
        if self.token_times:
            f, l = self.frames, self.logp
            self.frames = torch.full((h.shape[0], 2 * h.shape[1]), -1, dtype=f.dtype, device=f.device)
            self.logp = torch.zeros(h.shape[0], 2 * h.shape[1], dtype=l.dtype, device=l.device)
            self.frames[:, : h.shape[1]], self.logp[:, : h.shape[1]] = f, l

    def _begin(self, enc, frame_lengths, max_symbols, max_per_frame: int, max_hyp_len: int):
        """What the batched begins share: the outputs, then the torch mirror's state (-> None) or the engine's operands (->
        enc @ W1 + b1; `_keep`: the frame lengths and the symbol budget or None, alive while the launches read them)."""
        B, T = enc.shape[0], enc.shape[1]
        dev = enc.device
        self.B, self.T = B, T
        self._new_outputs(B, max_hyp_len, dev, 0, enc.dtype)
        frames = frame_lengths.to(device=dev, dtype=torch.int32)
        maxsym = None if max_symbols is None else max_symbols.to(device=dev, dtype=torch.int32)
        if not self.engine:
            return self._torch_begin(enc, frames, maxsym, int(max_per_frame))
        self._keep = (frames.contiguous(), maxsym.contiguous() if maxsym is not None else None)
        return (torch.matmul(enc.float(), self.W1) + self.b1).contiguous()

    def _begin_stream(self, slots: int, max_chunk_frames: int, max_per_frame: int, max_hyp_len: int, device):
        """What the streams' begins share: every slot finished, its outputs, and the torch mirror's state -> the device."""
        S, T = int(slots), int(max_chunk_frames)
        dev = self.W2.device if self.engine else (device if device is not None else self.joint.W2.device)
        self.B, self.T, self.Tc = S, T, T
        self._cap = int(max_per_frame)
        self._new_outputs(S, max_hyp_len, dev, 1, self.joint.W2.dtype)
        if self.engine:
            self.H = int(self.W1.shape[0])
        else:
            z = torch.zeros(S, dtype=torch.long, device=dev)
            self._frame_base = z.clone() if self.token_times else None
            self._t, self._n, self._nf, self._Tb, self._maxsym = z.clone(), z.clone(), z.clone(), z.clone(), z.clone()
            self._done = torch.ones(S, dtype=torch.bool, device=dev)
            self._fin = torch.ones(S, dtype=torch.bool, device=dev)
        return dev

    def _torch_begin(self, enc, frames, maxsym, max_per_frame):
        B, T = enc.shape[0], enc.shape[1]
        dev = enc.device
        self._enc = enc
        self._Tb = frames.clamp(0, T).long()
        self._maxsym = (torch.full((B,), 2**31 - 1, dtype=torch.long, device=dev) if maxsym is None else maxsym.clamp(min=0).long())
        self._cap = max_per_frame
        self._t = torch.zeros(B, dtype=torch.long, device=dev)
        self._n = torch.zeros(B, dtype=torch.long, device=dev)
        self._nf = torch.zeros(B, dtype=torch.long, device=dev)
        self._done = (self._Tb == 0) | (self._maxsym == 0)


class GreedyJoint(_GreedyEngineJoint):
    """The joint of the batched greedy decoder (decoding.greedy_decode_batch): one lattice cell per hypothesis and step, argmax,
    log-softmax of the decision and the decoder state in one pass.

    On an MI355X this is the ENGINE (include/rnnt.h compute_rnnt_greedy_begin / _step): the object owns the workspace (reused by
    the next decode when it is large enough) and the joint-unit padding of W1 / b1 / W2 (as joint_logits pads them; the vocabulary
    needs none: the step kernel skips padding columns itself).  The first Dense layer runs through torch.matmul on both sides:
    the encoder side once per decode, the prediction side once per step -- a [B, H] x [H, J] product, one hipBLASLt launch, where
    the library's dense path would be a second entry point and a workspace round trip for B rows.  CPU tensors and shapes the
    kernels do not take (joint sizes beyond 704 / 640) run the same state machine in torch on JointLoss.logits.

    begin(enc [B, T, H], frame_lengths [B], max_symbols [B] or None, max_per_frame, max_hyp_len) allocates the outputs
    (`hyps` [B, max_hyp_len] zero-filled, `lengths`, `scores`, `emitted`, `all_done`); step(pred [B, H]) advances every hypothesis
    by one decision and returns `emitted` (the symbol per row, or -1).  all_done[0]: 0 running, 1 finished, 2 paused on a full
    `hyps` buffer (grow_hyps() resumes them).

    token_times=True (compute_rnnt_greedy_step_timed): begin also allocates `frames` int32 [B, max_hyp_len] (-1 where no token is)
    and `logp` [B, max_hyp_len] (0 there): per token the encoder frame whose joint evaluation emitted it and the log-softmax of
    that decision (float32 on the engine; the dtype of `scores` on the torch route).  ids, lengths and scores are bitwise those
    of the untimed step."""

    # ---- engine
    def begin(self, enc, frame_lengths, max_symbols, max_per_frame: int, max_hyp_len: int):
        ep = self._begin(enc, frame_lengths, max_symbols, max_per_frame, max_hyp_len)
        if ep is None:
            return
        B, T = self.B, self.T
        frames, ms = self._keep
        with torch.cuda.device(enc.device):
            self._ws = _workspace(self._ws, _lib.greedy_workspace_bytes(T, B, self.Jp, self.V, self.dtype), enc.device)
            self._opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, self.blank, T, 1)
            st = _lib.load().compute_rnnt_greedy_begin(ep.data_ptr(), frames.data_ptr(), ptr(ms), self.W2.data_ptr(),
                                                       self.b2.data_ptr(), self.Jp, self.V, B, int(max_per_frame), self.dtype,
                                                       self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_greedy_begin")

    def step(self, pred=None, logit_stats=None, *, pred_proj=None):
        """pred [B, H]: the prediction network's output of every row -> emitted [B] (int32, -1 where nothing was emitted).
        pred_proj [B, Jp] instead of pred: that output already through W1 (PredictionStep); the step skips its matmul."""
        if not self.engine:
            return self._torch_step(pred, pred_proj)
        pp = torch.matmul(pred.float(), self.W1).contiguous() if pred_proj is None else _projected_operand(pred_proj, self.Jp)
        if self.token_times:
            st = _lib.load().compute_rnnt_greedy_step_timed(
                pp.data_ptr(), self.hyps.data_ptr(), self.frames.data_ptr(), self.logp.data_ptr(), self.hyps.shape[1],
                self.lengths.data_ptr(), self.scores.data_ptr(), self.emitted.data_ptr(), self.all_done.data_ptr(),
                ptr(logit_stats), ptr(self._frame_base), self.Jp, self.V, self.B, self.dtype, self._ws.data_ptr(), self._opts)
            _lib.check(st, "compute_rnnt_greedy_step_timed")
            return self.emitted
        st = _lib.load().compute_rnnt_greedy_step(pp.data_ptr(), self.hyps.data_ptr(), self.hyps.shape[1], self.lengths.data_ptr(),
                                                  self.scores.data_ptr(), self.emitted.data_ptr(), self.all_done.data_ptr(),
                                                  ptr(logit_stats), self.Jp, self.V, self.B, self.dtype, self._ws.data_ptr(),
                                                  self._opts)
        _lib.check(st, "compute_rnnt_greedy_step")
        return self.emitted

    # ---- torch composition: the same state machine (greedy_update_kernel) on JointLoss.logits
    def _torch_step(self, pred, pred_proj=None):
        B, T, N = self.B, self.T, self.hyps.shape[1]
        ar = torch.arange(B, device=self._enc.device)
        live = ~self._done & (self._n < self._maxsym.clamp(max=N))
        e = self._enc[ar, self._t.clamp(0, T - 1)]
        logits = _torch_cell_logits(self.joint, e, pred, pred_proj)
        k = torch.argmax(logits, dim=-1)
        M = logits.gather(1, k[:, None])[:, 0]
        lse = torch.logsumexp(logits, dim=-1)
        self.scores = torch.where(live, self.scores + (M - lse).to(self.scores.dtype), self.scores)
        emit = live & (k != self.blank)
        pos = self._n.clamp(max=N - 1)[:, None]
        self.hyps.scatter_(1, pos, torch.where(emit, k.to(torch.int32), self.hyps.gather(1, pos)[:, 0])[:, None])
        if self.token_times:  # (the frame of this decision: before the cursor moves on)
            fr = self._t if self._frame_base is None else self._t + self._frame_base
            self.frames.scatter_(1, pos, torch.where(emit, fr.to(torch.int32), self.frames.gather(1, pos)[:, 0])[:, None])
            self.logp.scatter_(1, pos, torch.where(emit, (M - lse).to(self.logp.dtype), self.logp.gather(1, pos)[:, 0])[:, None])
        self._n = self._n + emit.long()
        self._nf = torch.where(emit, self._nf + 1, self._nf)
        adv = live & ~emit  # blank: next frame
        if self._cap > 0:  # per-frame cap reached: next frame too
            adv = adv | (emit & (self._nf >= self._cap))
        self._t = self._t + adv.long()
        self._nf = torch.where(adv, torch.zeros_like(self._nf), self._nf)
        self._done = self._done | (live & ((self._t >= self._Tb) | (self._n >= self._maxsym)))
        self.lengths.copy_(self._n.to(torch.int32))
        self.emitted.copy_(torch.where(emit, k, torch.full_like(k, -1)).to(torch.int32))
        running, paused = ~self._done & (self._n < N), ~self._done & (self._n >= N)
        self.all_done.copy_(torch.where(running.any(), 0, torch.where(paused.any(), 2, 1)).to(torch.int32).reshape(1))
        return self.emitted


class GreedyStreamJoint(GreedyJoint):
    """The joint of the streaming greedy decoder (decoding.StreamingGreedyDecoder): GreedyJoint's step over `slots` streams whose
    encoder frames arrive chunk by chunk.

    On an MI355X this is the ENGINE (include/rnnt.h compute_rnnt_greedy_stream_begin / _feed, then compute_rnnt_greedy_step on
    the same workspace): the object owns the workspace (reused by the next begin when it is large enough) and W1 / b1 go into it,
    so the encoder side's projection runs in the library with a fixed summation order.  CPU tensors and shapes the kernels do not
    take run the same state machine in torch (GreedyJoint's torch step on JointLoss.logits).

    begin(slots, max_chunk_frames (encoder frames per feed), max_per_frame, max_hyp_len) leaves every slot finished;
    feed(enc [slots, Te, H], frames [slots], reset, final, max_symbols) hands every slot its chunk (device int32 vectors, or
    None); then step(pred_proj=...) until all_done[0] is 1, as for GreedyJoint."""

    def begin(self, slots: int, max_chunk_frames: int, max_per_frame: int, max_hyp_len: int, device=None):
        dev = self._begin_stream(slots, max_chunk_frames, max_per_frame, max_hyp_len, device)
        if not self.engine:
            return
        S, T = self.B, self.T
        self._frame_base = torch.zeros(S, dtype=torch.int32, device=dev) if self.token_times else None
        with torch.cuda.device(dev):
            nbytes = _lib.greedy_stream_workspace_bytes(T, S, self.H, self.Jp, self.V, self.dtype)
            self._ws = _workspace(self._ws, nbytes, dev)
            self._opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, self.blank, T, 1)
            st = _lib.load().compute_rnnt_greedy_stream_begin(self.W1.data_ptr(), self.b1.data_ptr(), self.W2.data_ptr(),
                                                              self.b2.data_ptr(), self.H, self.Jp, self.V, S, self.dtype,
                                                              self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_greedy_stream_begin")

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
            enc = _aligned16(enc.to(device=dev, dtype=torch.float32))
            if tuple(enc.shape) != (S, Te, self.H):
                raise ValueError(f"enc must be [{S}, frames, {self.H}], got {tuple(enc.shape)}")
        cv = lambda x: None if x is None else _device_i32(x, dev).reshape(S)  # noqa: E731
        fr, rs, fi, ms = cv(frames), cv(reset), cv(final), cv(max_symbols)
        self._feed_args = (enc, fr, rs, fi, ms)  # (alive until the launches have read them)
        if self.token_times:
            st = _lib.load().compute_rnnt_greedy_stream_feed_timed(
                ptr(enc) if Te > 0 else None, Te, fr.data_ptr(), ptr(rs), ptr(fi), ptr(ms), self._cap, self.lengths.data_ptr(),
                self.scores.data_ptr(), self.all_done.data_ptr(), self._frame_base.data_ptr(), self.H, self.Jp, self.V, S, self.dtype,
                self._ws.data_ptr(), self._opts)
            return _lib.check(st, "compute_rnnt_greedy_stream_feed_timed")
        st = _lib.load().compute_rnnt_greedy_stream_feed(ptr(enc) if Te > 0 else None, Te, fr.data_ptr(), ptr(rs), ptr(fi), ptr(ms),
                                                         self._cap, self.lengths.data_ptr(), self.scores.data_ptr(),
                                                         self.all_done.data_ptr(), self.H, self.Jp, self.V, S, self.dtype,
                                                         self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_greedy_stream_feed")

    def _torch_feed(self, enc, Te, frames, reset, final, max_symbols):
        S = self.B
        dev = self.hyps.device
        vec = lambda x, d: torch.full((S,), d, dtype=torch.long, device=dev) if x is None else torch.as_tensor(x).to(dev).reshape(S).long()  # noqa: E731
        rs, fi = vec(reset, 0) != 0, vec(final, 0) != 0
        ms = vec(max_symbols, 2**31 - 1).clamp(min=0)
        if self.token_times:  # (the frames of the chunk the slot leaves; a reset: frame 0 again)
            self._frame_base = torch.where(rs, 0, self._frame_base + self._Tb)
        self._n = torch.where(rs, 0, self._n)
        self.scores = torch.where(rs, torch.zeros_like(self.scores), self.scores)
        self._maxsym = torch.where(rs, ms, self._maxsym)
        self._fin = self._fin & ~rs
        finished = self._fin | (self._n >= self._maxsym)
        self._Tb = torch.where(finished, 0, vec(frames, 0).clamp(0, Te))
        self._fin = finished | fi
        self._t = torch.zeros_like(self._t)
        self._nf = torch.zeros_like(self._nf)
        self._done = self._Tb == 0
        H = self.joint.W1.shape[0]
        self._enc = enc if Te > 0 else torch.zeros(S, 1, H, dtype=self.joint.W1.dtype, device=dev)
        self.T = max(Te, 1)
        self.lengths.copy_(self._n.to(torch.int32))
        self.all_done.fill_(0 if bool((~self._done).any()) else 1)


class BeamJoint(_EngineJoint):
    """The joint of the batched beam search (decoding.beam_search_batch): per frame, the joint of every hypothesis of every beam,
    the candidate ranking, merging and the new beams in one pass ("modified" beam search, include/rnnt.h).

    On an MI355X this is the ENGINE (compute_rnnt_beam_begin / _step / _results), with GreedyJoint's workspace ownership and
    joint-unit padding.  CPU tensors and shapes the kernels do not take run the same state machine in torch on JointLoss.logits
    (in the model's dtype; per-utterance bookkeeping on the host).

    begin(enc [B, T, H], frame_lengths [B]); step(pred [B beam, H]) -> (parents, emitted) [B beam] int32; results() ->
    (hyps [B, beam, T] int32 zero-padded, lengths [B, beam] int32, scores [B, beam]), best first.

    token_times=True (compute_rnnt_beam_timed_*): results() returns two more, frames int32 [B, beam, T] (-1 padded) and logp
    [B, beam, T] (0 padded): per token the frame that emitted it and the log-softmax of that decision.  A hypothesis that
    absorbed merged candidates keeps the rows of its first-ranked member; its score is still the sum over the members.

    context=biasing.ContextGraph (compute_rnnt_beam_*_step_biased): every step ranks on logit + beta and carries the automaton
    state of every hypothesis; bias_states() -> int32 [B beam] after the last step.  results() of the OFFLINE search are
    finalised (score + fail_bias[state]: what a hypothesis left mid-phrase has not earned is taken back) and stably re-sorted
    by that score; the per-token log-probabilities stay the model's.

    lm=lm.NgramLM (compute_rnnt_beam_*_step_lm, include/rnnt_lm.h): shallow fusion of a back-off n-gram LM, in place of a context
    (one state word per hypothesis: lm together with context raises).  Every step ranks on logit + the LM's score of the token
    and carries the LM state of every hypothesis, which starts at the sentence start; lm_states() -> int32 [B beam].  results()
    of the OFFLINE search add the end-of-sentence score (final_score[state]) and are stably re-sorted, as with a context."""

    def __init__(self, joint: "JointLoss", beam: int = 4, joint_dtype: str = "auto", token_times: bool = False, context=None,
                 lm=None):
        if not 1 <= int(beam) <= 16:
            raise ValueError("BeamJoint: beam must be in 1 ... 16")
        self.K = int(beam)
        if lm is not None and context is not None:
            raise ValueError("lm= together with context=: a hypothesis carries one automaton state, take one of the two")
        self.context, self.lm = context, lm
        self._fsa = context if lm is None else lm  # the automaton of the torch mirror: either has row() and finalize()
        if context is not None and (context.blank != joint.blank_label or context.vocab_size != joint.W2.shape[1]):
            raise ValueError(f"context graph built for blank {context.blank} / {context.vocab_size} symbols, the joint has blank "
                             f"{joint.blank_label} / {joint.W2.shape[1]} symbols")
        if lm is not None and (lm.blank != joint.blank_label or lm.vocab_size != joint.W2.shape[1]):
            raise ValueError(f"LM built for blank {lm.blank} / {lm.vocab_size} symbols, the joint has blank "
                             f"{joint.blank_label} / {joint.W2.shape[1]} symbols")
        super().__init__(joint, joint_dtype, token_times)

    def begin(self, enc, frame_lengths):
        B, T = enc.shape[0], enc.shape[1]
        dev = enc.device
        self.B, self.T = B, T
        R = B * self.K
        self.parents = torch.arange(R, dtype=torch.int32, device=dev)
        self.emitted = torch.full((R,), -1, dtype=torch.int32, device=dev)
        self._bias_states = torch.zeros(R, dtype=torch.int32, device=dev)
        frames = frame_lengths.to(device=dev, dtype=torch.int32).contiguous()
        if not self.engine:
            return self._torch_begin(enc, frames)
        ep = (torch.matmul(enc.float(), self.W1) + self.b1).contiguous()
        self._keep = frames
        with torch.cuda.device(dev):
            size = _lib.beam_timed_workspace_bytes if self.token_times else _lib.beam_workspace_bytes
            nbytes = size(T, B, self.K, self.Jp, self.V, self.dtype)
            self._ws = _workspace(self._ws, nbytes, dev)
            self._opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, self.blank, T, 1)
            lib = _lib.load()
            fn = lib.compute_rnnt_beam_timed_begin if self.token_times else lib.compute_rnnt_beam_begin
            st = fn(ep.data_ptr(), frames.data_ptr(), self.W2.data_ptr(), self.b2.data_ptr(), self.Jp, self.V, B, self.K, self.dtype,
                    self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_beam_timed_begin" if self.token_times else "compute_rnnt_beam_begin")

    def step(self, pred=None, topk_logits=None, topk_symbols=None, lse=None, *, pred_proj=None):
        """pred [B beam, H]: the prediction network's output of every slot -> (parents, emitted), int32 [B beam].
        pred_proj [B beam, Jp] instead of pred: that output already through W1 (PredictionStep); the step skips its matmul."""
        if not self.engine:
            return self._torch_step(pred, pred_proj)
        pp = torch.matmul(pred.float(), self.W1).contiguous() if pred_proj is None else _projected_operand(pred_proj, self.Jp)
        lib = _lib.load()
        if self.context is not None:
            lib = _lib.load_bias()  # (include/rnnt_bias.h)
            fn = lib.compute_rnnt_beam_timed_step_biased if self.token_times else lib.compute_rnnt_beam_step_biased
            st = fn(pp.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(), ptr(topk_logits), ptr(topk_symbols), ptr(lse),
                    self.Jp, self.V, self.B, self.K, self.dtype, self._ws.data_ptr(), self._opts, self.context.byref(pp.device),
                    self._bias_states.data_ptr())
            _lib.check(st, "compute_rnnt_beam_timed_step_biased" if self.token_times else "compute_rnnt_beam_step_biased")
            return self.parents, self.emitted
        if self.lm is not None:
            lib = _lib.load_lm()  # (include/rnnt_lm.h)
            fn = lib.compute_rnnt_beam_timed_step_lm if self.token_times else lib.compute_rnnt_beam_step_lm
            st = fn(pp.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(), ptr(topk_logits), ptr(topk_symbols), ptr(lse),
                    self.Jp, self.V, self.B, self.K, self.dtype, self._ws.data_ptr(), self._opts, self.lm.byref(pp.device),
                    self._bias_states.data_ptr())
            _lib.check(st, "compute_rnnt_beam_timed_step_lm" if self.token_times else "compute_rnnt_beam_step_lm")
            return self.parents, self.emitted
        fn = lib.compute_rnnt_beam_timed_step if self.token_times else lib.compute_rnnt_beam_step
        st = fn(pp.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(), ptr(topk_logits), ptr(topk_symbols), ptr(lse),
                self.Jp, self.V, self.B, self.K, self.dtype, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_beam_timed_step" if self.token_times else "compute_rnnt_beam_step")
        return self.parents, self.emitted

    def bias_states(self):
        """int32 [B beam]: the context graph's state of every slot after the last step (zeros without a context)."""
        return self._bias_states

    def lm_states(self):
        """int32 [B beam]: the LM's state of every slot after the last step (zeros without an LM: the same word as bias_states)."""
        return self._bias_states

    def _finalised(self, out):
        """The offline results with a context or an LM: score + fail_bias[state] / final_score[state], every beam stably
        re-sorted by it."""
        if self._fsa is None:
            return out
        B, K = self.B, self.K
        scores = self._fsa.finalize(out[2], self._bias_states.reshape(B, K))
        scores, order = torch.sort(scores, dim=1, descending=True, stable=True)
        pick = lambda x: torch.gather(x, 1, order.reshape(B, K, *([1] * (x.dim() - 2))).expand_as(x))  # noqa: E731
        return (pick(out[0]), pick(out[1]), scores) + tuple(pick(x) for x in out[3:])

    def results(self):
        B, K, T = self.B, self.K, self.T
        if not self.engine:
            return self._finalised(self._torch_results())
        dev = self.parents.device
        hyps = torch.empty(B, K, T, dtype=torch.int32, device=dev)
        lengths = torch.empty(B, K, dtype=torch.int32, device=dev)
        scores = torch.empty(B, K, dtype=torch.float32, device=dev)
        if self.token_times:
            frames = torch.empty(B, K, T, dtype=torch.int32, device=dev)
            logp = torch.empty(B, K, T, dtype=torch.float32, device=dev)
            st = _lib.load().compute_rnnt_beam_timed_results(hyps.data_ptr(), lengths.data_ptr(), scores.data_ptr(), frames.data_ptr(),
                                                             logp.data_ptr(), self.Jp, self.V, B, K, self.dtype, self._ws.data_ptr(),
                                                             self._opts)
            _lib.check(st, "compute_rnnt_beam_timed_results")
            return self._finalised((hyps, lengths, scores, frames, logp))
        st = _lib.load().compute_rnnt_beam_results(hyps.data_ptr(), lengths.data_ptr(), scores.data_ptr(), self.Jp, self.V, B, K,
                                                   self.dtype, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_beam_results")
        return self._finalised((hyps, lengths, scores))

    # ---- torch composition: the same state machine (beam_select_kernel) on JointLoss.logits
    def _torch_begin(self, enc, frames):
        self._enc = enc
        self._Tb = [int(x) for x in frames.clamp(0, enc.shape[1]).tolist()]
        self._t = 0
        self._beams = [[((), 0.0)] for _ in range(self.B)]  # (tokens, float64 score), best first
        self._times = [[()] for _ in range(self.B)]  # token_times: per hypothesis its (frame, log-probability) pairs
        self._states = [[0] for _ in range(self.B)]  # context: per hypothesis its state in the graph
        self._sdtype = torch.promote_types(enc.dtype, torch.float32)

    def _torch_step(self, pred, pred_proj=None):
        B, K, V, blank = self.B, self.K, self.V, self.blank
        t = self._t
        self._t += 1
        parents = list(range(B * K))
        emitted = [-1] * (B * K)
        e = self._enc[:, min(t, self.T - 1)]  # [B, H]
        logits = _torch_cell_logits(self.joint, e.repeat_interleave(K, 0), pred, pred_proj)  # [B K, V]
        lse = torch.logsumexp(logits, dim=-1)
        top_l, top_v, bias = self._torch_top(logits)
        lse = lse.tolist()
        for b in range(B):
            if t < self._Tb[b]:
                self._torch_rank(b, top_l, top_v, lse, parents, emitted, frame=t, bias=bias)
        dev = self.parents.device
        self.parents = torch.tensor(parents, dtype=torch.int32, device=dev)
        self.emitted = torch.tensor(emitted, dtype=torch.int32, device=dev)
        self._torch_bias_states()
        return self.parents, self.emitted

    def _torch_top(self, logits):
        """Every row's top-K (logit, symbol) lists.  With a context: by the f32 key logit + beta (rule 2'), the logits raw, and
        bias = (beta, next state) of every listed symbol."""
        K = self.K
        if self._fsa is None:
            top_l, top_v = torch.sort(logits, dim=-1, descending=True, stable=True)  # (logit descending, symbol ascending)
            return top_l[:, :K].tolist(), top_v[:, :K].tolist(), None
        import numpy as np

        R = logits.shape[0]
        q = [0] * R
        for b, states in enumerate(self._states):
            q[b * K: b * K + len(states)] = states
        rows = [self._fsa.row(s) for s in q]
        beta = torch.from_numpy(np.stack([r[0] for r in rows])).to(logits.device)
        nxt = torch.from_numpy(np.stack([r[1] for r in rows])).to(logits.device)
        key = logits.float() + beta
        key = torch.where(torch.isnan(key), torch.full_like(key, -math.inf), key)  # (takes no part; the raw NaN drops it below)
        _, top_v = torch.sort(key, dim=-1, descending=True, stable=True)
        top_v = top_v[:, :K]
        return (torch.gather(logits, 1, top_v).tolist(), top_v.tolist(),
                (torch.gather(beta, 1, top_v).tolist(), torch.gather(nxt, 1, top_v).tolist()))

    def _torch_bias_states(self):
        if self._fsa is None:
            return
        q = [0] * (self.B * self.K)
        for b, states in enumerate(self._states):
            q[b * self.K: b * self.K + len(states)] = states
        self._bias_states = torch.tensor(q, dtype=torch.int32, device=self.parents.device)

    def _torch_rank(self, b, top_l, top_v, lse, parents, emitted, blank_l=None, cap=None, frame=0, bias=None):
        """One frame of beam b (rules 2 - 5 of include/rnnt.h) from every row's top-K lists and logsumexp; parents / emitted of
        its rows are filled in.  cap (the stream): a hypothesis of cap tokens offers its blank candidate (logit blank_l[r]) alone.
        frame: this frame's number for the (frame, log-probability) pairs; a merged hypothesis keeps its first member's.
        bias (a context): (beta, next state) beside every listed symbol -- beta joins the score, the state the hypothesis."""
        K, blank = self.K, self.blank
        beam = self._beams[b]
        states = self._states[b]
        cands = []
        for i, (y, s) in enumerate(beam):
            r = b * K + i
            full = cap is not None and len(y) >= cap
            offers = [(blank_l[r], blank)] if full else zip(top_l[r], top_v[r])
            extra = [(0.0, states[i])] * K if bias is None or full else zip(bias[0][r], bias[1][r])
            for (l, v), (be, nx) in zip(offers, extra):
                sc = s + (float(l) - lse[r]) + float(be) if bias is not None else s + (float(l) - lse[r])
                if sc == sc and sc > -math.inf:
                    cands.append((sc, i, v, float(l) - lse[r], nx))
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        taken = cands[:K]
        if not taken:
            return  # the beam is carried over
        times = self._times[b]
        merged = []  # [tokens, score, parent, emitted, (frame, log-probability) pairs, state]
        for sc, i, v, lp, nx in taken:
            y = beam[i][0] if v == blank else beam[i][0] + (v,)
            hit = next((m for m in merged if m[0] == y), None)
            if hit is None:
                merged.append([y, sc, i, -1 if v == blank else v, times[i] if v == blank else times[i] + ((frame, lp),), nx])
            else:
                hi, lo = max(hit[1], sc), min(hit[1], sc)
                hit[1] = hi + math.log1p(math.exp(lo - hi))
        merged.sort(key=lambda m: -m[1])  # (stable)
        self._beams[b] = [(m[0], m[1]) for m in merged]
        self._times[b] = [m[4] for m in merged]
        self._states[b] = [m[5] for m in merged]
        for k in range(len(merged)):
            parents[b * K + k], emitted[b * K + k] = b * K + merged[k][2], merged[k][3]

    def _torch_results(self):
        B, K, T = self.B, self.K, self.T
        hyps = torch.zeros(B, K, T, dtype=torch.int32)
        lengths = torch.zeros(B, K, dtype=torch.int32)
        scores = torch.full((B, K), -math.inf, dtype=torch.float64)
        for b, beam in enumerate(self._beams):
            for k, (y, s) in enumerate(beam):
                hyps[b, k, : len(y)] = torch.tensor(y, dtype=torch.int32)
                lengths[b, k], scores[b, k] = len(y), s
        dev = self.parents.device
        out = hyps.to(dev), lengths.to(dev), scores.to(device=dev, dtype=self._sdtype)
        return out + self._torch_times(T) if self.token_times else out

    def _torch_times(self, N):
        """(frames int32 [B, K, N] -1 padded, logp [B, K, N] 0 padded) of the mirror's beams."""
        frames = torch.full((self.B, self.K, N), -1, dtype=torch.int32)
        logp = torch.zeros(self.B, self.K, N, dtype=torch.float64)
        for b, rows in enumerate(self._times):
            for k, row in enumerate(rows):
                if row:
                    frames[b, k, : len(row)] = torch.tensor([f for f, _ in row], dtype=torch.int32)
                    logp[b, k, : len(row)] = torch.tensor([l for _, l in row], dtype=torch.float64)
        dev = self.parents.device
        return frames.to(dev), logp.to(device=dev, dtype=self._sdtype)


class BeamStreamJoint(BeamJoint):
    """The joint of the streaming beam search (decoding.StreamingBeamDecoder): BeamJoint's step over `slots` streams whose encoder
    frames arrive chunk by chunk, each slot keeping its beam from one feed to the next.

    On an MI355X this is the ENGINE (include/rnnt.h compute_rnnt_beam_stream_begin / _feed / _step / _results): the object owns
    the workspace and W1 / b1 go into it, so the encoder side's projection runs in the library with a fixed summation order.  CPU
    tensors and shapes the kernels do not take run the same state machine in torch, the capacity rule and `stable` included:
    the joint shapes GreedyJoint refuses, and what only the stream refuses at begin (an encoder width beyond 4096, or a workspace
    beyond the library's 2^31 index limits: 2 slots beam max_hyp_len tokens, slots max_chunk_frames joint units).

    begin(slots, max_chunk_frames (encoder frames per feed), max_hyp_len (the tokens a stream's hypothesis may hold)) leaves every
    slot finished with an empty beam; feed(enc [slots, Te, H], frames [slots], reset, final) hands every slot its chunk (int
    vectors, or None); then step(pred_proj=...) once per encoder frame of the longest chunk (host data: nothing is polled), each
    followed by a prediction-network step -- after the last frame too.  results() -> (hyps [slots, beam, max_hyp_len] zero-padded,
    lengths [slots, beam], scores [slots, beam], stable [slots]) at any time: stable = the common prefix of a slot's hypotheses,
    the tokens no later frame can change.

    token_times=True (compute_rnnt_beam_stream_timed_*): results() returns three more: frames int32 [slots, beam, max_hyp_len]
    (-1 padded; counted from the slot's reset across its chunks), logp [slots, beam, max_hyp_len] (0 padded) and timed_stable
    [slots] = the prefix on which the slot's hypotheses agree in token and emission frame (<= stable): tokens AND times final.

    context=biasing.ContextGraph: the biased steps; a reset returns a slot's states to the root and a finished slot keeps its
    states.  results() report the beam's own scores and order (a stream is never finalised: `stable` keeps its meaning);
    bias_states() -> int32 [slots beam], for a caller that wants context.finalize(scores, states) at a stream's end.

    lm=lm.NgramLM: the LM steps, as BeamJoint takes it; a reset returns a slot's states to state 0 (the sentence start) and a
    finished slot keeps its states.  lm_states() -> int32 [slots beam], for lm.finalize(scores, states) at a stream's end."""

    MAX_ROWS = 1024  # slots * beam: the prediction network's rows

    def begin(self, slots: int, max_chunk_frames: int, max_hyp_len: int, device=None):
        S, T, N, K = int(slots), int(max_chunk_frames), int(max_hyp_len), self.K
        if S < 1 or S * K > self.MAX_ROWS:
            raise ValueError(f"slots * beam must be in 1 ... {self.MAX_ROWS}, got {S} * {K}")
        if T < 1 or N < 1:
            raise ValueError("max_chunk_frames and max_hyp_len must be >= 1")
        dev = self.W2.device if self.engine else (device if device is not None else self.joint.W2.device)
        self.B, self.T, self.Tc, self.N = S, T, T, N
        self.parents = torch.arange(S * K, dtype=torch.int32, device=dev)
        self.emitted = torch.full((S * K,), -1, dtype=torch.int32, device=dev)
        self._bias_states = torch.zeros(S * K, dtype=torch.int32, device=dev)
        lib = _lib.load() if self.engine else None
        if self.engine:  # (the library's own answer: a size it refuses is a shape the stream kernels do not take)
            n = ctypes.c_size_t(0)
            size = lib.get_rnnt_beam_stream_timed_workspace_size if self.token_times else lib.get_rnnt_beam_stream_workspace_size
            self.engine = size(T, S, K, N, int(self.W1.shape[0]), self.Jp, self.V, self.dtype, ctypes.byref(n)) == _lib.STATUS_SUCCESS
        if not self.engine:
            self._beams = [[] for _ in range(S)]
            self._times = [[] for _ in range(S)]
            self._states = [[] for _ in range(S)]
            self._nsteps = [0] * S  # frames since the slot's reset
            self._fin, self._Tb, self._tc = [True] * S, [0] * S, [0] * S
            self._enc = None
            self._sdtype = torch.promote_types(self.joint.W2.dtype, torch.float32)
            return
        self.H = int(self.W1.shape[0])
        with torch.cuda.device(dev):
            size = _lib.beam_stream_timed_workspace_bytes if self.token_times else _lib.beam_stream_workspace_bytes
            nbytes = size(T, S, K, N, self.H, self.Jp, self.V, self.dtype)
            self._ws = _workspace(self._ws, nbytes, dev)
            self._opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, self.blank, T, 1)
            fn = lib.compute_rnnt_beam_stream_timed_begin if self.token_times else lib.compute_rnnt_beam_stream_begin
            st = fn(self.W1.data_ptr(), self.b1.data_ptr(), self.W2.data_ptr(), self.b2.data_ptr(), self.H, self.Jp, self.V, S, K, N,
                    self.dtype, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_beam_stream_timed_begin" if self.token_times else "compute_rnnt_beam_stream_begin")

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
            enc = _aligned16(enc.to(device=dev, dtype=torch.float32))
            if tuple(enc.shape) != (S, Te, self.H):
                raise ValueError(f"enc must be [{S}, frames, {self.H}], got {tuple(enc.shape)}")
        cv = lambda x: None if x is None else _device_i32(x, dev).reshape(S)  # noqa: E731
        fr, rs, fi = cv(frames), cv(reset), cv(final)
        self._feed_args = (enc, fr, rs, fi)  # (alive until the launches have read them)
        lib = _lib.load()
        fn = lib.compute_rnnt_beam_stream_timed_feed if self.token_times else lib.compute_rnnt_beam_stream_feed
        st = fn(ptr(enc) if Te > 0 else None, Te, fr.data_ptr(), ptr(rs), ptr(fi), self.H, self.Jp, self.V, S, self.K, self.N,
                self.dtype, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_beam_stream_timed_feed" if self.token_times else "compute_rnnt_beam_stream_feed")

    def step(self, pred=None, topk_logits=None, topk_symbols=None, lse=None, *, pred_proj=None):
        """One frame of every slot that has one left -> (parents, emitted), int32 [slots beam]; as BeamJoint.step."""
        if not self.engine:
            return self._torch_step(pred, pred_proj)
        pp = torch.matmul(pred.float(), self.W1).contiguous() if pred_proj is None else _projected_operand(pred_proj, self.Jp)
        lib = _lib.load()
        if self.context is not None:
            lib = _lib.load_bias()  # (include/rnnt_bias.h)
            fn = lib.compute_rnnt_beam_stream_timed_step_biased if self.token_times else lib.compute_rnnt_beam_stream_step_biased
            st = fn(pp.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(), ptr(topk_logits), ptr(topk_symbols), ptr(lse),
                    self.Jp, self.V, self.B, self.K, self.N, self.dtype, self._ws.data_ptr(), self._opts,
                    self.context.byref(pp.device), self._bias_states.data_ptr())
            _lib.check(st, "compute_rnnt_beam_stream_timed_step_biased" if self.token_times else "compute_rnnt_beam_stream_step_biased")
            return self.parents, self.emitted
        if self.lm is not None:
            lib = _lib.load_lm()  # (include/rnnt_lm.h)
            fn = lib.compute_rnnt_beam_stream_timed_step_lm if self.token_times else lib.compute_rnnt_beam_stream_step_lm
            st = fn(pp.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(), ptr(topk_logits), ptr(topk_symbols), ptr(lse),
                    self.Jp, self.V, self.B, self.K, self.N, self.dtype, self._ws.data_ptr(), self._opts,
                    self.lm.byref(pp.device), self._bias_states.data_ptr())
            _lib.check(st, "compute_rnnt_beam_stream_timed_step_lm" if self.token_times else "compute_rnnt_beam_stream_step_lm")
            return self.parents, self.emitted
        fn = lib.compute_rnnt_beam_stream_timed_step if self.token_times else lib.compute_rnnt_beam_stream_step
        st = fn(pp.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(), ptr(topk_logits), ptr(topk_symbols), ptr(lse),
                self.Jp, self.V, self.B, self.K, self.N, self.dtype, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_beam_stream_timed_step" if self.token_times else "compute_rnnt_beam_stream_step")
        return self.parents, self.emitted

    def results(self):
        S, K, N = self.B, self.K, self.N
        if not self.engine:
            return self._torch_results()
        dev = self.parents.device
        hyps = torch.empty(S, K, N, dtype=torch.int32, device=dev)
        lengths = torch.empty(S, K, dtype=torch.int32, device=dev)
        scores = torch.empty(S, K, dtype=torch.float32, device=dev)
        stable = torch.empty(S, dtype=torch.int32, device=dev)
        if self.token_times:
            frames = torch.empty(S, K, N, dtype=torch.int32, device=dev)
            logp = torch.empty(S, K, N, dtype=torch.float32, device=dev)
            tstable = torch.empty(S, dtype=torch.int32, device=dev)
            st = _lib.load().compute_rnnt_beam_stream_timed_results(
                hyps.data_ptr(), lengths.data_ptr(), scores.data_ptr(), stable.data_ptr(), frames.data_ptr(), logp.data_ptr(),
                tstable.data_ptr(), self.Jp, self.V, S, K, N, self.dtype, self._ws.data_ptr(), self._opts)
            _lib.check(st, "compute_rnnt_beam_stream_timed_results")
            return hyps, lengths, scores, stable, frames, logp, tstable
        st = _lib.load().compute_rnnt_beam_stream_results(hyps.data_ptr(), lengths.data_ptr(), scores.data_ptr(), stable.data_ptr(),
                                                          self.Jp, self.V, S, K, N, self.dtype, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_beam_stream_results")
        return hyps, lengths, scores, stable

    # ---- torch composition: the same state machine (beam_stream_feed_kernel, beam_select_kernel, beam_results_kernel)
    def _torch_feed(self, enc, Te, frames, reset, final):
        S = self.B
        vec = lambda x: [0] * S if x is None else [int(v) for v in torch.as_tensor(x).reshape(S).tolist()]  # noqa: E731
        fr, rs, fi = vec(frames), vec(reset), vec(final)
        for s in range(S):
            if rs[s]:
                self._beams[s], self._fin[s] = [((), 0.0)], False
                self._times[s], self._nsteps[s] = [()], 0
                self._states[s] = [0]
            self._tc[s] = 0
            if self._fin[s]:
                self._Tb[s] = 0
            else:
                self._Tb[s] = min(max(fr[s], 0), Te)
                self._fin[s] = fi[s] != 0
        self._enc = enc if Te > 0 else None

    def _torch_step(self, pred, pred_proj=None):
        S, K = self.B, self.K
        parents, emitted = list(range(S * K)), [-1] * (S * K)
        dev = self.parents.device
        live = [s for s in range(S) if self._tc[s] < self._Tb[s]]
        if live:
            Te = self._enc.shape[1]
            cur = torch.tensor([min(self._tc[s], Te - 1) for s in range(S)], device=self._enc.device)
            e = self._enc[torch.arange(S, device=self._enc.device), cur]  # [S, H]
            logits = _torch_cell_logits(self.joint, e.repeat_interleave(K, 0), pred, pred_proj)  # [S K, V]
            lse = torch.logsumexp(logits, dim=-1).tolist()
            top_l, top_v, bias = self._torch_top(logits)
            blank_l = logits[:, self.blank].tolist()
            for s in live:
                self._torch_rank(s, top_l, top_v, lse, parents, emitted, blank_l, self.N, frame=self._nsteps[s], bias=bias)
                self._tc[s] += 1
                self._nsteps[s] += 1
        self.parents = torch.tensor(parents, dtype=torch.int32, device=dev)
        self.emitted = torch.tensor(emitted, dtype=torch.int32, device=dev)
        self._torch_bias_states()
        return self.parents, self.emitted

    def _torch_results(self):
        S, K, N = self.B, self.K, self.N
        hyps = torch.zeros(S, K, N, dtype=torch.int32)
        lengths = torch.zeros(S, K, dtype=torch.int32)
        scores = torch.full((S, K), -math.inf, dtype=torch.float64)
        stable = torch.zeros(S, dtype=torch.int32)
        for s, beam in enumerate(self._beams):
            for k, (y, sc) in enumerate(beam):
                hyps[s, k, : len(y)] = torch.tensor(y, dtype=torch.int32)
                lengths[s, k], scores[s, k] = len(y), sc
            if beam:
                n = 0
                while all(n < len(y) for y, _ in beam) and all(y[n] == beam[0][0][n] for y, _ in beam):
                    n += 1
                stable[s] = n
        dev = self.parents.device
        out = hyps.to(dev), lengths.to(dev), scores.to(device=dev, dtype=self._sdtype), stable.to(dev)
        if not self.token_times:
            return out
        tstable = torch.zeros(S, dtype=torch.int32)
        for s, (beam, rows) in enumerate(zip(self._beams, self._times)):
            n = 0  # the prefix that agrees in token and frame
            while n < int(stable[s]) and all(r[n][0] == rows[0][n][0] for r in rows):
                n += 1
            tstable[s] = n
        return out + self._torch_times(N) + (tstable.to(dev),)


class MultiBeamJoint(_EngineJoint):
    """The joint of the batched beam search with SEVERAL symbols per frame (decoding.beam_search_batch(symbols_per_frame=E)): the
    time-synchronous search of include/rnnt_beam_multi.h, which states the rule.  Rows are 2 beam per utterance: slot k of the
    open list A is row b 2 beam + k, slot k of the closed list B row b 2 beam + beam + k.  One step is one round; a frame takes
    E + 1 of them.

    On an MI355X this is the ENGINE (compute_rnnt_multibeam_begin / _step / _results, libwarprnnt_multibeam.so).  CPU tensors and
    shapes the library refuses (the joint's, or more than 1024 rows) run the same rule in torch with float64 scores.

    begin(enc [B, T, H], frame_lengths [B]); step(pred [B 2 beam, H]) -> (parents, emitted) [B 2 beam] int32; results() ->
    (hyps [B, beam, max_hyp_len] int32 zero-padded, lengths [B, beam] int32, scores [B, beam]), list A, best first."""

    def __init__(self, joint: "JointLoss", beam: int = 4, symbols_per_frame: int = 2, max_hyp_len=None, joint_dtype: str = "auto"):
        if not 1 <= int(beam) <= 16:
            raise ValueError("MultiBeamJoint: beam must be in 1 ... 16")
        if not 1 <= int(symbols_per_frame) <= 8:
            raise ValueError("MultiBeamJoint: symbols_per_frame must be in 1 ... 8")
        if max_hyp_len is not None and int(max_hyp_len) < 1:
            raise ValueError("MultiBeamJoint: max_hyp_len must be at least 1")
        self.K, self.E = int(beam), int(symbols_per_frame)
        self.max_hyp_len = None if max_hyp_len is None else int(max_hyp_len)
        super().__init__(joint, joint_dtype, False)
        self._takes = self.engine  # (the joint's shape; begin adds the row limit)

    @property
    def rows_per_utterance(self) -> int:
        return 2 * self.K

    def begin(self, enc, frame_lengths):
        B, T = enc.shape[0], enc.shape[1]
        dev = enc.device
        self.B, self.T = B, T
        self.N = self.max_hyp_len if self.max_hyp_len is not None else max(1, T * self.E)
        R = B * 2 * self.K
        self.parents = torch.arange(R, dtype=torch.int32, device=dev)
        self.emitted = torch.full((R,), -1, dtype=torch.int32, device=dev)
        frames = frame_lengths.to(device=dev, dtype=torch.int32).contiguous()
        self.engine = self._takes and R <= 1024
        if not self.engine:
            return self._torch_begin(enc, frames)
        ep = (torch.matmul(enc.float(), self.W1) + self.b1).contiguous()
        self._keep = frames
        with torch.cuda.device(dev):
            nbytes = _lib.multibeam_workspace_bytes(T, B, self.K, self.E, self.N, self.Jp, self.V, self.dtype)
            self._ws = _workspace(self._ws, nbytes, dev)
            self._opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, self.blank, T, 1)
            st = _lib.load_multibeam().compute_rnnt_multibeam_begin(
                ep.data_ptr(), frames.data_ptr(), self.W2.data_ptr(), self.b2.data_ptr(), self.Jp, self.V, B, self.K, self.E, self.N,
                self.dtype, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_multibeam_begin")

    def step(self, pred=None, *, pred_proj=None):
        """pred [B 2 beam, H]: the prediction network's output of every row -> (parents, emitted), int32 [B 2 beam].
        pred_proj [B 2 beam, Jp] instead of pred: that output already through W1 (PredictionStep)."""
        if not self.engine:
            return self._torch_step(pred, pred_proj)
        pp = torch.matmul(pred.float(), self.W1).contiguous() if pred_proj is None else _projected_operand(pred_proj, self.Jp)
        st = _lib.load_multibeam().compute_rnnt_multibeam_step(
            pp.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(), self.Jp, self.V, self.B, self.K, self.E, self.N, self.dtype,
            self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_multibeam_step")
        return self.parents, self.emitted

    def results(self):
        B, K, N = self.B, self.K, self.N
        if not self.engine:
            return self._torch_results()
        dev = self.parents.device
        hyps = torch.empty(B, K, N, dtype=torch.int32, device=dev)
        lengths = torch.empty(B, K, dtype=torch.int32, device=dev)
        scores = torch.empty(B, K, dtype=torch.float32, device=dev)
        st = _lib.load_multibeam().compute_rnnt_multibeam_results(
            hyps.data_ptr(), lengths.data_ptr(), scores.data_ptr(), self.Jp, self.V, B, K, self.E, N, self.dtype, self._ws.data_ptr(),
            self._opts)
        _lib.check(st, "compute_rnnt_multibeam_results")
        return hyps, lengths, scores

    # ---- torch composition: the rule of include/rnnt_beam_multi.h on JointLoss.logits, float64 scores
    def _torch_begin(self, enc, frames):
        self._enc = enc
        self._Tb = [int(x) for x in frames.clamp(0, enc.shape[1]).tolist()]
        self._k = 0
        self._open = [[((), 0.0)] for _ in range(self.B)]  # (tokens, float64 score), in list order
        self._closed = [[] for _ in range(self.B)]
        self._sdtype = torch.promote_types(enc.dtype, torch.float32)

    def _torch_step(self, pred, pred_proj=None):
        B, K, E, blank = self.B, self.K, self.E, self.blank
        KR = 2 * K
        t, rnd = divmod(self._k, E + 1)
        self._k += 1
        parents = list(range(B * KR))
        emitted = [-1] * (B * KR)
        e = self._enc[:, min(t, self.T - 1)]  # [B, H]
        logits = _torch_cell_logits(self.joint, e.repeat_interleave(KR, 0), pred, pred_proj).double()  # [B 2K, V]
        lp = (logits - torch.logsumexp(logits, dim=-1, keepdim=True)).tolist()
        for b in range(B):
            if t >= self._Tb[b]:
                continue
            rb = b * KR
            A, Bl = self._open[b], self._closed[b]
            # closings: [sequence, score, the slot that holds its state]
            lst = [[y, s, K + j] for j, (y, s) in enumerate(Bl)]
            for i, (y, s) in enumerate(A):
                c = s + lp[rb + i][blank]
                if c != c or c == -math.inf:
                    continue
                hit = next((x for x in lst if x[0] == y), None)
                if hit is None:
                    lst.append([y, c, i])
                else:
                    hi, lo = max(hit[1], c), min(hit[1], c)
                    hit[1] = hi + math.log1p(math.exp(lo - hi))
            lst.sort(key=lambda x: -x[1])  # (stable)
            lst = lst[:K]
            if rnd < E:
                cands = []
                for i, (y, s) in enumerate(A):
                    if len(y) >= self.N:
                        continue
                    row = lp[rb + i]
                    for v in range(self.V):
                        sc = s + row[v]
                        if v != blank and sc == sc and sc > -math.inf:
                            cands.append((sc, i, v))
                cands.sort(key=lambda c: (-c[0], c[1], c[2]))
                cands = cands[:K]
                for k, (sc, i, v) in enumerate(cands):
                    parents[rb + k], emitted[rb + k] = rb + i, v
                for k, x in enumerate(lst):
                    parents[rb + K + k] = rb + x[2]
                self._open[b] = [(A[i][0] + (v,), sc) for sc, i, v in cands]
                self._closed[b] = [(x[0], x[1]) for x in lst]
            else:  # the frame turn
                for k, x in enumerate(lst):
                    parents[rb + k] = rb + x[2]
                self._open[b] = [(x[0], x[1]) for x in lst]
                self._closed[b] = []
        dev = self.parents.device
        self.parents = torch.tensor(parents, dtype=torch.int32, device=dev)
        self.emitted = torch.tensor(emitted, dtype=torch.int32, device=dev)
        return self.parents, self.emitted

    def _torch_results(self):
        B, K, N = self.B, self.K, self.N
        hyps = torch.zeros(B, K, N, dtype=torch.int32)
        lengths = torch.zeros(B, K, dtype=torch.int32)
        scores = torch.full((B, K), -math.inf, dtype=torch.float64)
        for b, beam in enumerate(self._open):
            for k, (y, s) in enumerate(beam):
                hyps[b, k, : len(y)] = torch.tensor(y, dtype=torch.int32)
                lengths[b, k], scores[b, k] = len(y), s
        dev = self.parents.device
        return hyps.to(dev), lengths.to(dev), scores.to(device=dev, dtype=self._sdtype)


class MultiBeamStreamJoint(MultiBeamJoint):
    """The joint of the streaming beam search with several symbols per frame (decoding.StreamingMultiBeamDecoder): the rule of
    MultiBeamJoint over `slots` streams whose encoder frames arrive chunk by chunk, each slot keeping its lists from one feed to
    the next.  include/rnnt_beam_multi_stream.h states the contract.

    On an MI355X this is the ENGINE (compute_rnnt_multibeam_stream_begin / _feed / _step / _results,
    libwarprnnt_multibeamstream.so): the object owns the workspace and W1 / b1 go into it, so the encoder side's projection runs in
    the library with a fixed summation order.  CPU tensors and shapes the library refuses run the same state machine in torch with
    float64 scores: the frame base, the frame rows (an entry a closing is added into keeps its own), both stable lengths.

    begin(slots, max_chunk_frames, max_hyp_len) leaves every slot finished with an empty beam; feed(enc [slots, Te, H], frames
    [slots], reset, final) hands every slot its chunk; then step(pred_proj=...) E + 1 times per encoder frame of the longest chunk,
    each followed by a prediction-network step over the slots' 2 beam rows.  results() -> (hyps [slots, beam, max_hyp_len]
    zero-padded, lengths, scores [slots, beam], stable [slots]); token_times=True adds frames int32 [slots, beam, max_hyp_len] (-1
    padded, counted from the slot's reset) and timed_stable [slots] (<= stable).  `stable` is final at frame boundaries only."""

    MAX_ROWS = 1024  # slots * 2 beam: the prediction network's rows

    def __init__(self, joint: "JointLoss", beam: int = 4, symbols_per_frame: int = 2, joint_dtype: str = "auto",
                 token_times: bool = False):
        super().__init__(joint, beam, symbols_per_frame, None, joint_dtype)
        self.token_times = bool(token_times)

    def begin(self, slots: int, max_chunk_frames: int, max_hyp_len: int, device=None):
        S, T, N, K = int(slots), int(max_chunk_frames), int(max_hyp_len), self.K
        if S < 1 or S * 2 * K > self.MAX_ROWS:
            raise ValueError(f"slots * 2 * beam must be in 1 ... {self.MAX_ROWS}, got {S} * 2 * {K}")
        if T < 1 or N < 1:
            raise ValueError("max_chunk_frames and max_hyp_len must be >= 1")
        self.engine = self._takes
        dev = self.W2.device if self.engine else (device if device is not None else self.joint.W2.device)
        self.B, self.T, self.Tc, self.N = S, T, T, N
        R = S * 2 * K
        self.parents = torch.arange(R, dtype=torch.int32, device=dev)
        self.emitted = torch.full((R,), -1, dtype=torch.int32, device=dev)
        if self.engine:  # (the library's own answer: a size it refuses is a shape the stream kernels do not take)
            n = ctypes.c_size_t(0)
            self.H = int(self.W1.shape[0])
            self.engine = _lib.load_multibeam_stream().get_rnnt_multibeam_stream_workspace_size(
                T, S, K, self.E, N, self.H, self.Jp, self.V, self.dtype, int(self.token_times), ctypes.byref(n)) == _lib.STATUS_SUCCESS
        if not self.engine:
            self._open = [[] for _ in range(S)]  # (tokens, float64 score, frames), in list order
            self._closed = [[] for _ in range(S)]
            self._fin, self._Tb, self._tc, self._rnd, self._base = [True] * S, [0] * S, [0] * S, [0] * S, [0] * S
            self._enc = None
            self._sdtype = torch.promote_types(self.joint.W2.dtype, torch.float32)
            return
        self._timed = int(self.token_times)
        with torch.cuda.device(dev):
            self._ws = _workspace(self._ws, n.value, dev)
            self._opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, self.blank, T, 1)
            st = _lib.load_multibeam_stream().compute_rnnt_multibeam_stream_begin(
                self.W1.data_ptr(), self.b1.data_ptr(), self.W2.data_ptr(), self.b2.data_ptr(), self.H, self.Jp, self.V, S, K, self.E, N,
                self.dtype, self._timed, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_multibeam_stream_begin")

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
            enc = _aligned16(enc.to(device=dev, dtype=torch.float32))
            if tuple(enc.shape) != (S, Te, self.H):
                raise ValueError(f"enc must be [{S}, frames, {self.H}], got {tuple(enc.shape)}")
        cv = lambda x: None if x is None else _device_i32(x, dev).reshape(S)  # noqa: E731
        fr, rs, fi = cv(frames), cv(reset), cv(final)
        self._feed_args = (enc, fr, rs, fi)  # (alive until the launches have read them)
        st = _lib.load_multibeam_stream().compute_rnnt_multibeam_stream_feed(
            ptr(enc) if Te > 0 else None, Te, fr.data_ptr(), ptr(rs), ptr(fi), self.H, self.Jp, self.V, S, self.K, self.E, self.N,
            self.dtype, self._timed, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_multibeam_stream_feed")

    def step(self, pred=None, *, pred_proj=None):
        """One round of every slot that has a frame left -> (parents, emitted), int32 [slots 2 beam]; as MultiBeamJoint.step."""
        if not self.engine:
            return self._torch_step(pred, pred_proj)
        pp = torch.matmul(pred.float(), self.W1).contiguous() if pred_proj is None else _projected_operand(pred_proj, self.Jp)
        st = _lib.load_multibeam_stream().compute_rnnt_multibeam_stream_step(
            pp.data_ptr(), self.parents.data_ptr(), self.emitted.data_ptr(), self.Jp, self.V, self.B, self.K, self.E, self.N, self.dtype,
            self._timed, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_multibeam_stream_step")
        return self.parents, self.emitted

    def results(self):
        S, K, N = self.B, self.K, self.N
        if not self.engine:
            return self._torch_results()
        dev = self.parents.device
        hyps = torch.empty(S, K, N, dtype=torch.int32, device=dev)
        lengths = torch.empty(S, K, dtype=torch.int32, device=dev)
        scores = torch.empty(S, K, dtype=torch.float32, device=dev)
        stable = torch.empty(S, dtype=torch.int32, device=dev)
        frames = torch.empty(S, K, N, dtype=torch.int32, device=dev) if self.token_times else None
        tstable = torch.empty(S, dtype=torch.int32, device=dev) if self.token_times else None
        st = _lib.load_multibeam_stream().compute_rnnt_multibeam_stream_results(
            hyps.data_ptr(), lengths.data_ptr(), scores.data_ptr(), stable.data_ptr(), ptr(frames), ptr(tstable), self.Jp, self.V, S, K,
            self.E, N, self.dtype, self._timed, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_multibeam_stream_results")
        if self.token_times:
            return hyps, lengths, scores, stable, frames, tstable
        return hyps, lengths, scores, stable

    # ---- torch composition: the same state machine (tsd_stream_feed_kernel, multibeam_select_body.h, tsd_stream_results_kernel)
    def _torch_feed(self, enc, Te, frames, reset, final):
        S = self.B
        vec = lambda x: [0] * S if x is None else [int(v) for v in torch.as_tensor(x).reshape(S).tolist()]  # noqa: E731
        fr, rs, fi = vec(frames), vec(reset), vec(final)
        for s in range(S):
            if rs[s]:
                self._open[s], self._fin[s], self._base[s] = [((), 0.0, ())], False, 0
            elif not self._fin[s]:
                self._base[s] += self._Tb[s]
            self._closed[s] = []  # (round 0: what a feed finds unfinished of a frame's rounds is dropped)
            self._tc[s], self._rnd[s] = 0, 0
            if self._fin[s]:
                self._Tb[s] = 0
            else:
                self._Tb[s] = min(max(fr[s], 0), Te)
                self._fin[s] = fi[s] != 0
        self._enc = enc if Te > 0 else None

    def _torch_step(self, pred, pred_proj=None):
        S, K, E, blank = self.B, self.K, self.E, self.blank
        KR = 2 * K
        parents, emitted = list(range(S * KR)), [-1] * (S * KR)
        dev = self.parents.device
        live = [s for s in range(S) if self._tc[s] < self._Tb[s]]
        if live:
            Te = self._enc.shape[1]
            cur = torch.tensor([min(self._tc[s], Te - 1) for s in range(S)], device=self._enc.device)
            e = self._enc[torch.arange(S, device=self._enc.device), cur]  # [S, H]
            logits = _torch_cell_logits(self.joint, e.repeat_interleave(KR, 0), pred, pred_proj).double()  # [S 2K, V]
            lp = (logits - torch.logsumexp(logits, dim=-1, keepdim=True)).tolist()
        for b in live:
            rb, rnd, frame = b * KR, self._rnd[b], self._base[b] + self._tc[b]
            A, Bl = self._open[b], self._closed[b]
            # closings: [sequence, score, the slot that holds its state, its frames]; a hit keeps its own frames
            lst = [[y, s, K + j, f] for j, (y, s, f) in enumerate(Bl)]
            for i, (y, s, f) in enumerate(A):
                c = s + lp[rb + i][blank]
                if c != c or c == -math.inf:
                    continue
                hit = next((x for x in lst if x[0] == y), None)
                if hit is None:
                    lst.append([y, c, i, f])
                else:
                    hi, lo = max(hit[1], c), min(hit[1], c)
                    hit[1] = hi + math.log1p(math.exp(lo - hi))
            lst.sort(key=lambda x: -x[1])  # (stable)
            lst = lst[:K]
            if rnd < E:
                cands = []
                for i, (y, s, f) in enumerate(A):
                    if len(y) >= self.N:
                        continue
                    row = lp[rb + i]
                    for v in range(self.V):
                        sc = s + row[v]
                        if v != blank and sc == sc and sc > -math.inf:
                            cands.append((sc, i, v))
                cands.sort(key=lambda c: (-c[0], c[1], c[2]))
                cands = cands[:K]
                for k, (sc, i, v) in enumerate(cands):
                    parents[rb + k], emitted[rb + k] = rb + i, v
                for k, x in enumerate(lst):
                    parents[rb + K + k] = rb + x[2]
                self._open[b] = [(A[i][0] + (v,), sc, A[i][2] + (frame,)) for sc, i, v in cands]
                self._closed[b] = [(x[0], x[1], x[3]) for x in lst]
                self._rnd[b] = rnd + 1
            else:  # the frame turn
                for k, x in enumerate(lst):
                    parents[rb + k] = rb + x[2]
                self._open[b] = [(x[0], x[1], x[3]) for x in lst]
                self._closed[b] = []
                self._rnd[b] = 0
                self._tc[b] += 1
        self.parents = torch.tensor(parents, dtype=torch.int32, device=dev)
        self.emitted = torch.tensor(emitted, dtype=torch.int32, device=dev)
        return self.parents, self.emitted

    def _torch_results(self):
        S, K, N = self.B, self.K, self.N
        hyps = torch.zeros(S, K, N, dtype=torch.int32)
        frames = torch.full((S, K, N), -1, dtype=torch.int32)
        lengths = torch.zeros(S, K, dtype=torch.int32)
        scores = torch.full((S, K), -math.inf, dtype=torch.float64)
        stable = torch.zeros(S, dtype=torch.int32)
        tstable = torch.zeros(S, dtype=torch.int32)
        for s, beam in enumerate(self._open):
            for k, (y, sc, f) in enumerate(beam):
                hyps[s, k, : len(y)] = torch.tensor(y, dtype=torch.int32)
                frames[s, k, : len(y)] = torch.tensor(f, dtype=torch.int32)
                lengths[s, k], scores[s, k] = len(y), sc
            if beam:
                shortest = min(len(y) for y, _, _ in beam)
                n = 0
                while n < shortest and all(y[n] == beam[0][0][n] for y, _, _ in beam):
                    n += 1
                stable[s] = n
                n = 0
                while n < shortest and all(y[n] == beam[0][0][n] and f[n] == beam[0][2][n] for y, _, f in beam):
                    n += 1
                tstable[s] = n
        dev = self.parents.device
        out = hyps.to(dev), lengths.to(dev), scores.to(device=dev, dtype=self._sdtype), stable.to(dev)
        if not self.token_times:
            return out
        return out + (frames.to(dev), tstable.to(dev))


def _aligned16(x: torch.Tensor) -> torch.Tensor:
    x = x.detach().contiguous()
    return x if x.data_ptr() % 16 == 0 else x.clone()


def _device_i32(x, dev) -> torch.Tensor:
    """x (a tensor, a list or an array) as a contiguous int32 tensor on dev; host data goes through pinned memory without a
    host synchronisation."""
    if isinstance(x, torch.Tensor) and x.device == dev:
        return _aligned16(x.to(torch.int32))
    t = torch.as_tensor(x).to(torch.int32).contiguous()
    if t.device.type == "cpu" and dev.type == "cuda":
        t = t.pin_memory()
    return _aligned16(t.to(dev, non_blocking=True))


def _pred_step(pred_net, tokens: torch.Tensor, states):
    """One symbol through the prediction network for every row: tokens [B] -> (output [B, H], new states)."""
    y = pred_net.embed(tokens.long()[:, None])
    new = []
    for blk, st in zip(pred_net.blocks, states):
        y, hc = blk.lstm(y, st)
        y = blk.norm(blk.drop(y))
        new.append(hc)
    return y[:, 0, :], new


class TorchPredictionStep:
    """The prediction network of every decoder row stepped with the model's own modules, in the shape of PredictionStep:
    begin(rows) runs the start token 0 from zero state; step(emitted [rows], parents [rows] or None) gives every row the output
    and LSTM state of row parents[r] (None: its own), then the rows that emitted a symbol (emitted >= 0) advance by it and the
    others keep both.  Both return `g` [rows, H], the network's UNPROJECTED output: what a joint step takes as `pred`."""

    projected = False  # (a joint step takes the output as pred=, not as pred_proj=)

    def __init__(self, pred_net, device):
        self.net, self.device = pred_net, device

    def begin(self, rows: int, mask=None) -> torch.Tensor:
        """mask [rows] given: only those rows restart; the others keep their output and state."""
        g0, st0 = _pred_step(self.net, torch.zeros(rows, dtype=torch.int32, device=self.device), [None] * len(self.net.blocks))
        if mask is None:
            self.g, self.states = g0, st0
        else:
            self._take(mask, g0, st0, self.g, self.states)
        return self.g

    def step(self, emitted: torch.Tensor, parents=None) -> torch.Tensor:
        g, states = self.g, self.states
        if parents is not None:
            idx = parents.to(g.device).long()
            g = g[idx]
            states = [(h[:, idx], c[:, idx]) for h, c in states]
        emitted = emitted.to(g.device)
        g2, states2 = _pred_step(self.net, emitted.clamp(min=0), states)
        self._take(emitted >= 0, g2, states2, g, states)
        return self.g

    def _take(self, mask, g2, states2, g, states):
        self.g = torch.where(mask[:, None], g2, g)
        self.states = [(torch.where(mask[None, :, None], h2, h), torch.where(mask[None, :, None], c2, c))
                       for (h2, c2), (h, c) in zip(states2, states)]


class PredictionStep:
    """One prediction-network step for every decoder row, through the joint's first Dense layer: the `pred_proj` that
    GreedyJoint.step / BeamJoint.step take as `pred_proj=`.

    On an MI355X this is the ENGINE (include/rnnt.h compute_rnnt_prednet_begin / _step): begin packs the current weights into
    the workspace (the object owns it; the next decode reuses it when it is large enough), zeroes every row's state and runs the
    start token 0; each step advances the rows with emitted >= 0 from row parents[r]'s state (parents None: their own) and
    carries the others over.  CPU tensors, models that are not float32 and shapes the kernels do not take run the same state
    machine in torch (a TorchPredictionStep, then matmul(W1)).

    pred_net: model.PredictionNetwork (embedding + single-layer LSTM blocks with LayerNorm); W1 [out, Jp]: the joint's first
    Dense layer zero-padded to the decoder's joint units (GreedyJoint.W1 on the engine).  begin(rows) -> pred_proj [rows, Jp];
    step(emitted [rows] int32, parents [rows] int32 or None) -> pred_proj (the same tensor, overwritten by the next step)."""

    MAX_ROWS, MAX_BLOCKS, MAX_WIDTH = 1024, 8, 4096
    projected = True  # (a joint step takes the output as pred_proj=)

    def __init__(self, pred_net, W1: torch.Tensor):
        self.net = pred_net
        self.W1 = W1.detach()
        self.Jp = int(W1.shape[1])
        self.engine = self._engine_takes()
        self._ws = None

    def _engine_takes(self) -> bool:
        net, W1 = self.net, self.W1
        blocks = list(net.blocks)
        if not W1.is_cuda or not 1 <= len(blocks) <= self.MAX_BLOCKS or self.Jp % 64 != 0 or not 64 <= self.Jp <= 704:
            return False
        tensors = [W1, net.embed.weight]
        width = net.embed.embedding_dim
        if width > self.MAX_WIDTH:
            return False
        for blk in blocks:
            lstm, norm = blk.lstm, blk.norm
            if lstm.num_layers != 1 or lstm.bidirectional or not lstm.bias or lstm.input_size != width:
                return False
            out = lstm.proj_size or lstm.hidden_size
            if lstm.hidden_size > self.MAX_WIDTH or out > self.MAX_WIDTH or not norm.elementwise_affine or norm.bias is None:
                return False
            if tuple(norm.normalized_shape) != (out,):
                return False
            tensors += list(lstm.parameters()) + [norm.weight, norm.bias]
            width = out
        if W1.shape[0] != width:
            return False
        return all(t.dtype == torch.float32 and t.device == W1.device for t in tensors)

    def begin(self, rows: int) -> torch.Tensor:
        self.R = int(rows)
        self._use_engine = self.engine and 1 <= self.R <= self.MAX_ROWS
        dev = self.W1.device
        if not self._use_engine:
            self._torch = TorchPredictionStep(self.net, dev)
            return self._project(self._torch.begin(self.R))
        net = self.net
        keep = [_aligned16(net.embed.weight), _aligned16(self.W1)]
        blocks = (_lib.rnntPrednetBlock * len(net.blocks))()
        for b, blk in zip(blocks, net.blocks):
            lstm, norm = blk.lstm, blk.norm
            w = [_aligned16(x) for x in (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, norm.weight, norm.bias)]
            wr = _aligned16(lstm.weight_hr_l0) if lstm.proj_size else None
            keep += w + ([wr] if wr is not None else [])
            b.W_ih, b.W_hh, b.b_ih, b.b_hh = (x.data_ptr() for x in w[:4])
            b.W_hr = None if wr is None else wr.data_ptr()
            b.ln_weight, b.ln_bias = w[4].data_ptr(), w[5].data_ptr()
            b.hidden, b.proj, b.ln_eps = lstm.hidden_size, lstm.proj_size or lstm.hidden_size, float(norm.eps)
        self._blocks, self._keep = blocks, keep
        self.E, self.V = net.embed.embedding_dim, net.embed.num_embeddings
        self._n = 0
        with torch.cuda.device(dev):
            nbytes = _lib.prednet_workspace_bytes(blocks, self.E, self.V, self.Jp, self.R)
            self._ws = _workspace(self._ws, nbytes, dev)
            self.pred_proj = torch.empty(self.R, self.Jp, dtype=torch.float32, device=dev)
            self._opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, 1, 1)
            st = _lib.load().compute_rnnt_prednet_begin(keep[0].data_ptr(), blocks, len(blocks), self.E, self.V, keep[1].data_ptr(),
                                                        self.Jp, self.R, self.pred_proj.data_ptr(), self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_prednet_begin")
        self._n = 1
        return self.pred_proj

    def step(self, emitted: torch.Tensor, parents=None) -> torch.Tensor:
        if not self._use_engine:
            return self._project(self._torch.step(emitted, parents))
        dev = self.pred_proj.device
        em = emitted.to(device=dev, dtype=torch.int32).contiguous()
        pa = None if parents is None else parents.to(device=dev, dtype=torch.int32).contiguous()
        self._args = (em, pa)  # (alive until the launch has read them)
        st = _lib.load().compute_rnnt_prednet_step(em.data_ptr(), ptr(pa), self.pred_proj.data_ptr(),
                                                   self._blocks, len(self._blocks), self.E, self.V, self.Jp, self.R,
                                                   self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_prednet_step")
        self._n += 1
        return self.pred_proj

    def reset(self, mask) -> torch.Tensor:
        """Restart the rows where mask [rows] (bool or int) is set: zero state, then the start token 0 -- what begin runs for
        every row (compute_rnnt_prednet_reset on the engine).  The other rows keep their state and pred_proj.  -> pred_proj."""
        if not self._use_engine:
            m = torch.as_tensor(mask, device=self._torch.device).reshape(self.R).bool()
            return self._project(self._torch.begin(self.R, m))
        m = _device_i32(mask, self.pred_proj.device).reshape(self.R)
        self._args = (m,)
        st = _lib.load().compute_rnnt_prednet_reset(m.data_ptr(), self.pred_proj.data_ptr(), self._blocks, len(self._blocks), self.E,
                                                    self.V, self.Jp, self.R, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_prednet_reset")
        self._n += 1
        return self.pred_proj

    def state(self):
        """Every block's current (r [rows, proj], c [rows, hidden]): torch's (h, c) of the LSTM (views on the engine, valid until
        the next step)."""
        if not self._use_engine:
            return [(h[0], c[0]) for h, c in self._torch.states]
        R = self.R
        a64 = lambda n: (n + 63) // 64 * 64  # noqa: E731  (the workspace layout of include/rnnt.h)
        sizes = [(R * b.proj, R * b.hidden) for b in self._blocks]
        S = sum(a64(p) + a64(c) for p, c in sizes)
        f = self._ws.view(torch.float32)
        off = (self._n & 1) * S
        out = []
        for (p, c), b in zip(sizes, self._blocks):
            out.append((f[off: off + p].view(R, b.proj), f[off + a64(p): off + a64(p) + c].view(R, b.hidden)))
            off += a64(p) + a64(c)
        return out

    def _project(self, g):
        return torch.matmul(g.to(self.W1.dtype), self.W1)


class EncoderStream:
    """The encoder's forward pass (model.Encoder, inference) with its LSTM state carried from one run to the next, so that a long
    input may be encoded in chunks: begin(rows, max_frames), then run(mel_chunk [rows, frames, feat]) -> enc_chunk [rows,
    ceil(frames / f), out_width] any number of times.  Each run pads its own odd tail at the TimeReduction, as the module does
    per call; chunks whose lengths are multiples of f, except the last, give the output of one run over the whole input.

    On an MI355X this is the ENGINE (include/rnnt.h compute_rnnt_encoder_begin / _run): begin packs the current weights and the
    BatchNorm's running statistics into the workspace (the object owns it; the next begin reuses it when it is large enough) and
    zeroes every row's state.  CPU tensors, models that are not float32, a BatchNorm without running statistics, multi-layer or
    bidirectional LSTMs and shapes the kernels do not take run the same state machine in torch: BatchNorm (eval) -> per block
    nn.LSTM(x, (h, c)) with the carried state -> LayerNorm, TimeReduction of the chunk after block reduction_index."""

    MAX_ROWS, MAX_LAYERS, MAX_WIDTH, MAX_FACTOR, MAX_FRAMES = 1024, 16, 4096, 16, 1 << 20

    def __init__(self, encoder):
        self.enc = encoder
        self.factor = int(encoder.reduce.factor)
        self.ridx = int(encoder.reduction_index)
        self.engine = self._engine_takes()
        self._ws = None

    def _engine_takes(self) -> bool:
        enc = self.enc
        bn, blocks = enc.input_norm, list(enc.blocks)
        if bn.running_mean is None or bn.running_var is None or bn.weight is None or bn.bias is None:
            return False
        dev = bn.weight.device
        if dev.type != "cuda" or not 1 <= len(blocks) <= self.MAX_LAYERS or not 0 <= self.ridx < len(blocks) - 1:
            return False
        if not 1 <= self.factor <= self.MAX_FACTOR:
            return False
        width = bn.num_features
        tensors = [bn.weight, bn.bias, bn.running_mean, bn.running_var]
        for i, blk in enumerate(blocks):
            lstm, norm = blk.lstm, blk.norm
            if width > self.MAX_WIDTH:
                return False
            if lstm.num_layers != 1 or lstm.bidirectional or not lstm.bias or lstm.input_size != width or not lstm.batch_first:
                return False
            out = lstm.proj_size or lstm.hidden_size
            if lstm.hidden_size > self.MAX_WIDTH or out > self.MAX_WIDTH or not norm.elementwise_affine or norm.bias is None:
                return False
            if tuple(norm.normalized_shape) != (out,):
                return False
            tensors += list(lstm.parameters()) + [norm.weight, norm.bias]
            width = out * (self.factor if i == self.ridx else 1)
        return all(t.dtype == torch.float32 and t.device == dev for t in tensors)

    def begin(self, rows: int, max_frames: int) -> None:
        self.R, self.Tmax = int(rows), int(max_frames)
        self._use_engine = self.engine and 1 <= self.R <= self.MAX_ROWS and 1 <= self.Tmax <= self.MAX_FRAMES
        enc = self.enc
        if not self._use_engine:
            dev = enc.input_norm.weight.device if enc.input_norm.weight is not None else next(enc.parameters()).device
            dt = next(enc.blocks[0].lstm.parameters()).dtype
            self._states = []
            for blk in enc.blocks:
                lstm = blk.lstm
                self._states.append((torch.zeros(1, self.R, lstm.proj_size or lstm.hidden_size, dtype=dt, device=dev),
                                     torch.zeros(1, self.R, lstm.hidden_size, dtype=dt, device=dev)))
            return
        bn = enc.input_norm
        dev = bn.weight.device
        keep = [_aligned16(x) for x in (bn.running_mean, bn.running_var, bn.weight, bn.bias)]
        blocks = (_lib.rnntPrednetBlock * len(enc.blocks))()
        for b, blk in zip(blocks, enc.blocks):
            lstm, norm = blk.lstm, blk.norm
            w = [_aligned16(x) for x in (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, norm.weight, norm.bias)]
            wr = _aligned16(lstm.weight_hr_l0) if lstm.proj_size else None
            keep += w + ([wr] if wr is not None else [])
            b.W_ih, b.W_hh, b.b_ih, b.b_hh = (x.data_ptr() for x in w[:4])
            b.W_hr = None if wr is None else wr.data_ptr()
            b.ln_weight, b.ln_bias = w[4].data_ptr(), w[5].data_ptr()
            b.hidden, b.proj, b.ln_eps = lstm.hidden_size, lstm.proj_size or lstm.hidden_size, float(norm.eps)
        self._blocks, self._keep = blocks, keep
        self.F, self.bn_eps = bn.num_features, float(bn.eps)
        with torch.cuda.device(dev):
            nbytes = _lib.encoder_workspace_bytes(blocks, self.F, self.ridx, self.factor, self.R, self.Tmax)
            self._ws = _workspace(self._ws, nbytes, dev)
            self._opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, 1, 1)
            st = _lib.load().compute_rnnt_encoder_begin(blocks, len(blocks), self.F, *(x.data_ptr() for x in keep[:4]), self.bn_eps,
                                                        self.ridx, self.factor, self.R, self.Tmax, self._ws.data_ptr(), self._opts)
        _lib.check(st, "compute_rnnt_encoder_begin")

    @torch.no_grad()
    def run(self, mel_chunk: torch.Tensor, row_frames=None, reset=None) -> torch.Tensor:
        """mel_chunk [rows, frames, feat] -> the encoder output of these frames [rows, ceil(frames / f), out_width].

        Ragged rows (compute_rnnt_encoder_run_rows): rows where reset [rows] is set start from zero state; row r advances over
        its first row_frames[r] frames only (a row with 0 frames keeps its state), reads zeros beyond them at the reduction,
        and its output is zero past ceil(row_frames[r] / f) frames.  Both None: every row runs every frame (today's run)."""
        if mel_chunk.dim() != 3 or mel_chunk.shape[0] != self.R:
            raise ValueError(f"mel_chunk must be [{self.R}, frames, feat], got {tuple(mel_chunk.shape)}")
        rows = row_frames is not None or reset is not None
        if not self._use_engine:
            return self._torch_run_rows(mel_chunk, row_frames, reset) if rows else self._torch_run(mel_chunk)
        T = int(mel_chunk.shape[1])
        if mel_chunk.shape[2] != self.F or not 1 <= T <= self.Tmax:
            raise ValueError(f"mel_chunk must be [{self.R}, 1 ... {self.Tmax}, {self.F}], got {tuple(mel_chunk.shape)}")
        dev = self._ws.device
        x = _aligned16(mel_chunk.to(device=dev, dtype=torch.float32))
        out = torch.empty(self.R, -(-T // self.factor), self._blocks[len(self._blocks) - 1].proj, dtype=torch.float32, device=dev)
        self._x = x  # (alive until the launches have read it)
        if rows:
            rf = _device_i32([T] * self.R if row_frames is None else row_frames, dev).reshape(self.R)
            rs = None if reset is None else _device_i32(reset, dev).reshape(self.R)
            self._rows = (rf, rs)
            st = _lib.load().compute_rnnt_encoder_run_rows(x.data_ptr(), T, rf.data_ptr(), ptr(rs),
                                                           out.data_ptr(), self._blocks, len(self._blocks), self.F, self.bn_eps,
                                                           self.ridx, self.factor, self.R, self.Tmax, self._ws.data_ptr(), self._opts)
            _lib.check(st, "compute_rnnt_encoder_run_rows")
            return out
        st = _lib.load().compute_rnnt_encoder_run(x.data_ptr(), T, out.data_ptr(), self._blocks, len(self._blocks), self.F,
                                                  self.bn_eps, self.ridx, self.factor, self.R, self.Tmax, self._ws.data_ptr(),
                                                  self._opts)
        _lib.check(st, "compute_rnnt_encoder_run")
        return out

    def state(self):
        """Every block's current (r [rows, proj], c [rows, hidden]): torch's (h, c) of the LSTM (views on the engine, valid until
        the next run)."""
        if not self._use_engine:
            return [(h[0], c[0]) for h, c in self._states]
        R = self.R
        a64 = lambda n: (n + 63) // 64 * 64  # noqa: E731  (the workspace layout of include/rnnt.h)
        f = self._ws.view(torch.float32)
        off, out = 0, []
        for b in self._blocks:
            p, c = R * b.proj, R * b.hidden
            out.append((f[off: off + p].view(R, b.proj), f[off + a64(p): off + a64(p) + c].view(R, b.hidden)))
            off += a64(p) + a64(c)
        return out

    # ---- torch composition
    def _torch_run(self, x):
        enc = self.enc
        bn = enc.input_norm
        dt = self._states[0][0].dtype
        x = x.to(device=self._states[0][0].device, dtype=dt)
        x = torch.nn.functional.batch_norm(x.transpose(1, 2), bn.running_mean, bn.running_var, bn.weight, bn.bias,
                                           bn.running_mean is None, 0.0, bn.eps).transpose(1, 2)
        states = []
        for i, (blk, st) in enumerate(zip(enc.blocks, self._states)):
            y, st = blk.lstm(x, st)
            states.append(st)
            x = blk.norm(y)
            if i == enc.reduction_index:
                x = enc.reduce(x)
        self._states = states
        return x

    def _torch_run_rows(self, x, row_frames, reset):
        """The ragged run in torch: packed sequences give every row its own last frame's state."""
        enc = self.enc
        bn = enc.input_norm
        R, T = x.shape[0], x.shape[1]
        dt, dev = self._states[0][0].dtype, self._states[0][0].device
        x = x.to(device=dev, dtype=dt)
        if reset is not None:
            m = torch.as_tensor(reset).to(dev).reshape(R).bool()
            self._states = [(torch.where(m[None, :, None], 0.0, h), torch.where(m[None, :, None], 0.0, c)) for h, c in self._states]
        rf = [T] * R if row_frames is None else [min(max(int(v), 0), T) for v in torch.as_tensor(row_frames).reshape(R).tolist()]
        f = self.factor
        width = enc.blocks[len(enc.blocks) - 1].lstm.proj_size or enc.blocks[len(enc.blocks) - 1].lstm.hidden_size
        out = torch.zeros(R, -(-T // f), width, dtype=dt, device=dev)
        live = [r for r in range(R) if rf[r] > 0]
        if not live:
            return out
        idx = torch.tensor(live, device=dev)
        lens = torch.tensor([rf[r] for r in live])
        y = x[idx]
        y = torch.nn.functional.batch_norm(y.transpose(1, 2), bn.running_mean, bn.running_var, bn.weight, bn.bias,
                                           bn.running_mean is None, 0.0, bn.eps).transpose(1, 2)
        pack = torch.nn.utils.rnn
        states = []
        for i, (blk, (h, c)) in enumerate(zip(enc.blocks, self._states)):
            Tl = y.shape[1]
            p, (h2, c2) = blk.lstm(pack.pack_padded_sequence(y, lens, batch_first=True, enforce_sorted=False),
                                   (h[:, idx].contiguous(), c[:, idx].contiguous()))
            y, _ = pack.pad_packed_sequence(p, batch_first=True, total_length=Tl)
            y = blk.norm(y) * (torch.arange(Tl)[None, :] < lens[:, None]).to(device=dev, dtype=dt)[:, :, None]
            states.append((h.index_copy(1, idx, h2), c.index_copy(1, idx, c2)))
            if i == enc.reduction_index:
                y = enc.reduce(y)
                lens = (lens + f - 1) // f
        self._states = states
        out[idx] = y
        return out
