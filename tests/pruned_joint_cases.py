"""The fused joint on the pruned band (include/rnnt_pruned_joint.h compute_rnnt_joint_loss_pruned), restated in float64 from its
contract, and the input builders the CPU and GPU tests share.  Nothing of the code under test is imported.  Plain and slow: the
lattice is tests/pruned_cases.py's restatement, the joint around it is one slot at a time.

    logits(t, s, :) = tanh(enc[t] + pred[u]) @ W2 + b2,  u = sb[t] + s, for PRESENT slots (t < T, 0 <= u <= L) alone: an absent
    slot reads no row of enc or pred (the tests put NaN there)
    dlogits = pruned_cases.utterance's gradients (cost_scale and lambda applied)
    dz(t, s) = (dlogits(t, s) @ W2^T) (1 - h^2);  d_enc[t] = sum_s dz;  d_pred[u] = sum over the slots that are cell (., u) of dz
    dW2 = sum h^T dlogits;  db2 = sum dlogits
An utterance with an out-of-range length: T clamped into [1, maxT], L into [0, maxU - 1], NaN cost and NaN dlogits on the present
slots of the clamped lattice."""
import numpy as np

from tests import pruned_cases as pc

TOPOLOGIES = pc.TOPOLOGIES
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -(2 ** 31)


def band_logits(enc, pred, W2, b2, sb, T, L, S):
    """One utterance: (x [maxT, S, V] float64 with zeros in absent slots, h [maxT, S, J] likewise, u [maxT, S] with -1 for absent)."""
    maxT, J = enc.shape
    V = W2.shape[1]
    W, bias = np.asarray(W2, np.float64), np.asarray(b2, np.float64)
    x, h, uu = np.zeros((maxT, S, V)), np.zeros((maxT, S, J)), -np.ones((maxT, S), np.int64)
    for t in range(T):
        for s in range(S):
            u = int(sb[t]) + s
            if 0 <= u <= L:
                uu[t, s] = u
                h[t, s] = np.tanh(np.asarray(enc[t], np.float64) + np.asarray(pred[u], np.float64))
                x[t, s] = h[t, s] @ W + bias
    return x, h, uu


def loss_and_grads(enc, pred, W2, b2, s_begin, labels, il, ll, S, lam=0.0, cost_scale=None, blank=0, topology="standard"):
    """Batched, ragged: dict(costs [B], d_enc [B, T, J], d_pred [B, U, J], dW2 [J, V], db2 [V]) in float64; the gradients are
    those of sum_b cost_scale[b] cost_b."""
    enc, pred = np.asarray(enc), np.asarray(pred)
    B, maxT, J = enc.shape
    maxU, V = pred.shape[1], np.asarray(W2).shape[1]
    W = np.asarray(W2, np.float64)
    cs = np.ones(B) if cost_scale is None else np.broadcast_to(np.asarray(cost_scale, np.float64), (B,))
    out = dict(costs=np.zeros(B), d_enc=np.zeros((B, maxT, J)), d_pred=np.zeros((B, maxU, J)), dW2=np.zeros((J, V)), db2=np.zeros(V))
    for b in range(B):
        T, L = int(il[b]), int(ll[b])
        bad = T < 1 or T > maxT or L < 0 or L > maxU - 1
        T, L = min(max(T, 1), maxT), min(max(L, 0), maxU - 1)
        x, h, uu = band_logits(enc[b], pred[b], W2, b2, s_begin[b], T, L, S)
        if bad:
            c, g = np.nan, np.where((uu >= 0)[:, :, None], np.nan, 0.0) * np.ones((1, 1, V))
        else:
            c, g = pc.utterance(x, s_begin[b], labels[b], T, L, lam, blank, topology)
        g = g * cs[b]
        out["costs"][b] = c
        for t, s in zip(*np.nonzero(uu >= 0)):
            dz = (g[t, s] @ W.T) * (1.0 - h[t, s] ** 2)
            out["d_enc"][b, t] += dz
            out["d_pred"][b, uu[t, s]] += dz
            out["dW2"] += np.outer(h[t, s], g[t, s])
            out["db2"] += g[t, s]
    return out


GRAD_KEYS = ("d_enc", "d_pred", "dW2", "db2")


def composed_logits(enc, pred, W2, b2, s_begin, il, ll, S):
    """The band's logits [B, T, S, V] float64 as the composed route forms them (zeros in absent slots), for the existing
    restatement and mirror."""
    enc, pred = np.asarray(enc), np.asarray(pred)
    B, maxT, _ = enc.shape
    out = np.zeros((B, maxT, S, np.asarray(W2).shape[1]))
    for b in range(B):
        out[b] = band_logits(enc[b], pred[b], W2, b2, s_begin[b], int(il[b]), int(ll[b]), S)[0]
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------
def poison_rows(enc, pred, il, ll):
    """NaN in the rows of enc beyond T_b and of pred beyond L_b (in place; lengths clamped into the tensors); returns both."""
    for b in range(enc.shape[0]):
        enc[b, min(max(int(il[b]), 1), enc.shape[1]):] = np.nan
        pred[b, min(max(int(ll[b]), 0), pred.shape[1] - 1) + 1:] = np.nan
    return enc, pred


def straight_ranges(T, S, il, ll):
    """Band positions on the straight line from 0 to hi = max(0, L_b + 1 - S), int32 [B, T]: steps of 0 and 1 as long as
    L_b <= T_b - 1.  With L_b <= T_b - 2 the band connects on both lattices (u(t) = min(t, sb[t] + S - 1) is a path of the
    modified one); S = 1 on the standard lattice connects only without labels."""
    sb = np.zeros((len(il), T), np.int32)
    for b in range(len(il)):
        Tb, hi = int(il[b]), max(0, int(ll[b]) + 1 - S)
        sb[b] = np.minimum((np.arange(T) * hi) // max(Tb - 1, 1), hi)
    return sb


def joint_case(B, T, L, S, J, V, seed, sigma=1.0, w_scale=1.0, blank=0, ragged=True, steps=None, line=False):
    """A random case: dict(enc [B, T, J], pred [B, L + 1, J] with NaN beyond the lengths, W2, b2, sb, labels [B, L], il, ll, S).
    N(0, sigma) projections, glorot W2 times w_scale, monotone band positions from (0, 0) to the end: a random staircase, or with
    `line` straight_ranges with every L_b <= T_b - 2 (L <= T - 2 is the caller's)."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, V - 1, size=(B, max(L, 1))).astype(np.int32)
    labels += labels >= blank
    il, ll = np.full(B, T, np.int32), np.full(B, L, np.int32)
    if ragged and B > 1:
        il[1:] = rng.integers((T + 1) // 2, T + 1, size=B - 1)
        ll[1:] = rng.integers(L // 2, L + 1, size=B - 1)
    if line:
        ll = np.minimum(ll, il - 2).astype(np.int32)
        assert ll.min() >= 0
    sb = straight_ranges(T, S, il, ll) if line else pc.staircase_ranges(rng, B, T, S, il, ll, steps)
    enc = (rng.normal(size=(B, T, J)) * sigma).astype(np.float32)
    pred = (rng.normal(size=(B, max(L, 1) + 1, J)) * sigma).astype(np.float32)
    lim = np.sqrt(6.0 / (J + V))
    W2 = (rng.uniform(-lim, lim, size=(J, V)) * w_scale).astype(np.float32)
    b2 = (0.1 * w_scale * rng.normal(size=V)).astype(np.float32)
    poison_rows(enc, pred, il, ll)
    return dict(enc=enc, pred=pred, W2=W2, b2=b2, sb=sb, labels=labels, il=il, ll=ll, S=S)


def hostile_case(J=64, V=28, seed=300):
    """The ranges of tests/test_pruned_loss_gpu.py's hostile case (B10 T10 S4 L7) around projections: steps of S, decreasing,
    negative, past L, INT32_MAX / MIN, short and empty utterances, L = 0, T = 1."""
    B, T, S, L = 10, 10, 4, 7
    rng = np.random.default_rng(seed)
    labels = rng.integers(1, V, size=(B, L)).astype(np.int32)
    il, ll = np.full(B, T, np.int32), np.full(B, L, np.int32)
    good = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4], np.int32)
    sb = np.tile(good, (B, 1))
    sb[0] = [0, 0, 0, 4, 4, 4, 4, 4, 4, 4]           # a step of S: the bands do not touch
    sb[1] = [0, 1, 2, 1, 2, 3, 2, 3, 4, 4]           # decreasing in places
    sb[2] = [-2, -1, 0, 1, 1, 2, 2, 3, 4, 4]         # negative: cell (0, 0) sits at slot 2
    sb[3] = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]           # past L: the last rows have fewer and fewer present cells, then none
    sb[4] = [0, 1, 1, INT32_MAX, 2, 3, INT32_MIN, 4, 4, 4]
    ll[5] = 1                                        # L_b < S - 1
    sb[5] = 0
    il[6], ll[6] = 1, 0                              # T_b = 1
    sb[6] = 0
    ll[7] = 0                                        # L_b = 0
    sb[7] = [0, -1, -3, 0, 0, -2, 0, 0, -3, 0]
    il[8], ll[8] = 3, 6                              # L_b > T_b: no path on the modified lattice
    sb[8] = [0, 2, 3, 3, 3, 3, 3, 3, 3, 3]
    il[9], ll[9] = 1, 1                              # T_b = 1 with a label: the modified lattice's last frame emits it
    sb[9] = 0
    enc = rng.normal(size=(B, T, J)).astype(np.float32)
    pred = rng.normal(size=(B, L + 1, J)).astype(np.float32)
    lim = np.sqrt(6.0 / (J + V))
    W2 = rng.uniform(-lim, lim, size=(J, V)).astype(np.float32)
    b2 = (0.1 * rng.normal(size=V)).astype(np.float32)
    poison_rows(enc, pred, il, ll)
    return dict(enc=enc, pred=pred, W2=W2, b2=b2, sb=sb, labels=labels, il=il, ll=ll, S=S)


def touched_rows(sb, il, ll, S, maxT, maxU):
    """(enc rows [B, maxT], pred rows [B, maxU]) bool: the rows some present slot points at; gradients elsewhere are exact zeros."""
    m = pc.present_mask(sb, np.clip(il, 1, maxT), np.clip(ll, 0, maxU - 1), S)
    u = np.asarray(sb, np.int64)[:, :, None] + np.arange(S)[None, None, :]
    rows_e = m.any(axis=2)
    rows_p = np.zeros((m.shape[0], maxU), bool)
    bb, tt, ss = np.nonzero(m)
    rows_p[bb, u[bb, tt, ss]] = True
    return rows_e, rows_p
