"""The fused TDT joint (include/rnnt_tdt_joint.h compute_rnnt_joint_loss_tdt), restated in float64 from its contract, and the input
builders the CPU and GPU tests share.  Nothing of the code under test is imported.  Plain and slow: the lattice is
tests/tdt_cases.py's restatement, the joint around it is NumPy on the live cells.

    logits(t, u, :) = tanh(enc[t] + pred[u]) @ W2 + b2 for LIVE cells (t < T, u <= L) alone: a padded cell reads no row of enc or
    pred (the tests put NaN there); the first V columns are the token head, the last D the duration head
    dlogits = tdt_cases.loss_and_grad's gradients (cost_scale applied)
    dz(t, u) = (dlogits(t, u) @ W2^T) (1 - h^2);  d_enc[t] = sum_u dz;  d_pred[u] = sum_t dz
    dW2 = sum h^T dlogits;  db2 = sum dlogits
An utterance with an out-of-range length: T clamped into [1, maxT], L into [0, maxU - 1], NaN cost and NaN dlogits on the live
cells of the clamped lattice."""
import numpy as np

from tests import tdt_cases as tc

GRAD_KEYS = ("d_enc", "d_pred", "dW2", "db2")


def live_logits(enc, pred, W2, b2, T, L):
    """One utterance: (x [T, L + 1, V + D], h [T, L + 1, J]) in float64 from the first T rows of enc and L + 1 rows of pred."""
    e, p = np.asarray(enc[:T], np.float64), np.asarray(pred[: L + 1], np.float64)
    h = np.tanh(e[:, None, :] + p[None, :, :])
    return h @ np.asarray(W2, np.float64) + np.asarray(b2, np.float64), h


def composed_logits(enc, pred, W2, b2, il, ll):
    """The logits [B, maxT, maxU, V + D] float64 as the composed route forms them, zeros in padded cells."""
    enc, pred = np.asarray(enc), np.asarray(pred)
    B, maxT, _ = enc.shape
    maxU = pred.shape[1]
    out = np.zeros((B, maxT, maxU, np.asarray(W2).shape[1]))
    for b in range(B):
        T, L = min(max(int(il[b]), 1), maxT), min(max(int(ll[b]), 0), maxU - 1)
        out[b, :T, : L + 1] = live_logits(enc[b], pred[b], W2, b2, T, L)[0]
    return out


def loss_and_grads(enc, pred, W2, b2, labels, il, ll, durations, blank=0, sigma=0.0, cost_scale=None):
    """Batched, ragged: dict(costs [B], d_enc [B, T, J], d_pred [B, U, J], dW2 [J, V + D], db2 [V + D]) in float64; the gradients
    are those of sum_b cost_scale[b] cost_b."""
    enc, pred = np.asarray(enc), np.asarray(pred)
    B, maxT, J = enc.shape
    maxU, R = pred.shape[1], np.asarray(W2).shape[1]
    W = np.asarray(W2, np.float64)
    cs = np.ones(B) if cost_scale is None else np.broadcast_to(np.asarray(cost_scale, np.float64), (B,))
    out = dict(costs=np.zeros(B), d_enc=np.zeros((B, maxT, J)), d_pred=np.zeros((B, maxU, J)), dW2=np.zeros((J, R)), db2=np.zeros(R))
    for b in range(B):
        T, L = int(il[b]), int(ll[b])
        bad = T < 1 or T > maxT or L < 0 or L > maxU - 1
        T, L = min(max(T, 1), maxT), min(max(L, 0), maxU - 1)
        x, h = live_logits(enc[b], pred[b], W2, b2, T, L)
        if bad:
            c, g = np.nan, np.full(x.shape, np.nan)
        else:
            c, g = tc.loss_and_grad(x[None], np.asarray(labels[b])[None], [T], [L], durations, blank, sigma, [cs[b]])
            c, g = c[0], g[0]
        out["costs"][b] = c
        dz = (g @ W.T) * (1.0 - h * h)  # [T, L + 1, J]
        out["d_enc"][b, :T] = dz.sum(axis=1)
        out["d_pred"][b, : L + 1] = dz.sum(axis=0)
        out["dW2"] += np.einsum("tuj,tuv->jv", h, g)
        out["db2"] += g.sum(axis=(0, 1))
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------
def poison_rows(enc, pred, il, ll):
    """NaN in the rows of enc beyond T_b and of pred beyond L_b (in place; lengths clamped into the tensors); returns both."""
    for b in range(enc.shape[0]):
        enc[b, min(max(int(il[b]), 1), enc.shape[1]):] = np.nan
        pred[b, min(max(int(ll[b]), 0), pred.shape[1] - 1) + 1:] = np.nan
    return enc, pred


def joint_case(lengths, J, V, D, seed, sigma=1.0, w_scale=1.0, blank=0, poison=True):
    """A random case with one utterance per (T_b, L_b) of `lengths`: dict(enc [B, T, J], pred [B, L + 1, J], W2 [J, V + D],
    b2, labels [B, max(L, 1)], il, ll), T = max T_b, L = max L_b.  N(0, sigma) projections, glorot W2 times w_scale, labels that
    avoid the blank; with `poison`, NaN in the rows beyond the lengths."""
    rng = np.random.default_rng(seed)
    B = len(lengths)
    T, L = max(t for t, _ in lengths), max(l for _, l in lengths)
    labels = rng.integers(0, V - 1, size=(B, max(L, 1))).astype(np.int32)
    labels += labels >= blank
    il = np.array([t for t, _ in lengths], np.int32)
    ll = np.array([l for _, l in lengths], np.int32)
    enc = (rng.normal(size=(B, T, J)) * sigma).astype(np.float32)
    pred = (rng.normal(size=(B, L + 1, J)) * sigma).astype(np.float32)
    lim = np.sqrt(6.0 / (J + V + D))
    W2 = (rng.uniform(-lim, lim, size=(J, V + D)) * w_scale).astype(np.float32)
    b2 = (0.1 * w_scale * rng.normal(size=V + D)).astype(np.float32)
    if poison:
        poison_rows(enc, pred, il, ll)
    return dict(enc=enc, pred=pred, W2=W2, b2=b2, labels=labels, il=il, ll=ll)
