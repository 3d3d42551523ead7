"""The modified (one symbol per frame) transducer lattice of include/rnnt_modified.h compute_rnnt_loss_modified, restated in float64
NumPy from its equations, and the input builders the CPU and GPU tests share.

Per utterance, T frames, L labels, lp = log_softmax(x), nodes (t, u), 0 <= t <= T, 0 <= u <= L:
    alpha(0,0) = 0, else -inf;   alpha(t,u) = logaddexp(alpha(t-1,u) + lp(t-1,u,blank), alpha(t-1,u-1) + lp(t-1,u-1,y_{u-1}))
    ln P = alpha(T,L),  cost = -ln P
    beta(T,L) = 0, else -inf;    beta(t,u) = logaddexp(lp(t,u,blank) + beta(t+1,u), lp(t,u,y_u) + beta(t+1,u+1))
    e_b = exp(alpha + lp(blank) + beta(t+1,u) - ln P),  e_l = exp(alpha + lp(y_u) + beta(t+1,u+1) - ln P)  (0 at u = L)
    grads[t,u,v] = cs ((e_b + e_l + lambda e_l) softmax(x)[v] - [v == blank] e_b - [v == y_u] (1 + lambda) e_l)
L > T: no path -- cost +inf, gradients zero."""
import itertools

import numpy as np

from tests import fastemit_cases as fc


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def edges(x, labels, blank=0):
    """x [T, L+1, V] -> (lp, lpb [T, L+1], lpl [T, L]); labels outside [0, V) are clamped."""
    T, U, V = x.shape
    lp = log_softmax(x)
    y = np.clip(np.asarray(labels[: U - 1], np.int64), 0, V - 1)
    lpl = lp[:, np.arange(U - 1), y] if U > 1 else np.zeros((T, 0))
    return lp, lp[:, :, blank], lpl, y


def alphas(lpb, lpl):
    T, U = lpb.shape
    a = np.full((T + 1, U), -np.inf)
    a[0, 0] = 0.0
    for t in range(1, T + 1):
        a[t] = a[t - 1] + lpb[t - 1]
        a[t, 1:] = np.logaddexp(a[t, 1:], a[t - 1, : U - 1] + lpl[t - 1])
    return a


def betas(lpb, lpl):
    T, U = lpb.shape
    b = np.full((T + 1, U), -np.inf)
    b[T, U - 1] = 0.0
    for t in range(T - 1, -1, -1):
        b[t] = lpb[t] + b[t + 1]
        b[t, : U - 1] = np.logaddexp(b[t, : U - 1], lpl[t] + b[t + 1, 1:])
    return b


def band(T, L):
    """bool [T, L+1]: the live cells a path can pass through (u <= t and L - u <= T - t)."""
    t, u = np.arange(T)[:, None], np.arange(L + 1)[None, :]
    return (u <= t) & (L - u <= T - t)


def utterance(x, labels, lam=0.0, blank=0):
    """One utterance with exact lengths: x [T, L+1, V] logits -> (cost, grads [T, L+1, V]) in float64."""
    x = np.asarray(x, np.float64)
    T, U, V = x.shape
    lp, lpb, lpl, y = edges(x, labels, blank)
    with np.errstate(invalid="ignore"):
        a, b = alphas(lpb, lpl), betas(lpb, lpl)
    ll = a[T, U - 1]
    if ll == -np.inf:
        return np.inf, np.zeros((T, U, V))
    e_b = np.exp(a[:T] + lpb + b[1:] - ll)
    e_l = np.zeros((T, U))
    e_l[:, : U - 1] = np.exp(a[:T, : U - 1] + lpl + b[1:, 1:] - ll)
    g = (e_b + e_l + lam * e_l)[:, :, None] * np.exp(lp)
    g[:, :, blank] -= e_b
    if U > 1:
        np.subtract.at(g, (np.arange(T)[:, None], np.arange(U - 1)[None, :], y[None, :]), (1.0 + lam) * e_l[:, : U - 1])
    g[~band(T, U - 1)] = 0.0  # (no mass there: e_b = e_l = 0 already)
    return -ll, g


def loss_and_grad(acts, labels, il, ll, lam=0.0, cost_scale=None, blank=0):
    """Batched, ragged: (costs [B], grads [B, T, U, V]); padded cells are zeros; grads carry cost_scale."""
    acts = np.asarray(acts)
    B, T, U, V = acts.shape
    costs, grads = np.zeros(B), np.zeros((B, T, U, V))
    cs = np.ones(B) if cost_scale is None else np.broadcast_to(np.asarray(cost_scale, np.float64), (B,))
    for i in range(B):
        Tb, Ub = int(il[i]), int(ll[i]) + 1
        c, g = utterance(acts[i, :Tb, :Ub], np.asarray(labels[i])[: Ub - 1], lam, blank)
        costs[i] = c
        grads[i, :Tb, :Ub] = cs[i] * g
    return costs, grads


def band_mask(shape, il, ll):
    """bool [B, T, U]: True inside the band of each utterance; padded and out-of-band cells False."""
    B, T, U = shape
    m = np.zeros((B, T, U), bool)
    for i in range(B):
        Tb, Lb = int(il[i]), int(ll[i])
        m[i, :Tb, : Lb + 1] = band(Tb, Lb)
    return m


def brute_force_cost(x, labels, blank=0):
    """-ln of the sum over all C(T, L) paths: a path picks the L frames that emit a label, every other frame emits a blank."""
    x = np.asarray(x, np.float64)
    T, U, V = x.shape
    L = U - 1
    lp = log_softmax(x)
    total = -np.inf
    for emit in itertools.combinations(range(T), L):
        u, s = 0, 0.0
        for t in range(T):
            if t in emit:
                s += lp[t, u, labels[u]]
                u += 1
            else:
                s += lp[t, u, blank]
        total = np.logaddexp(total, s)
    return -total


# ---- inputs -------------------------------------------------------------------------------------------------------------
def full_case(B, T, L, V, seed, sigma=1.0, blank=0):
    """Full lengths; labels avoid the blank."""
    rng = np.random.default_rng(seed)
    acts = (rng.normal(size=(B, T, L + 1, V)) * sigma).astype(np.float32)
    labels = rng.integers(0, V - 1, size=(B, max(L, 1))).astype(np.int32)
    labels += labels >= blank
    return acts, labels, np.full(B, T, np.int32), np.full(B, L, np.int32)


def trained_like_case(B, T, L, V, seed):
    """tests/fastemit_cases.trained_like_case (one dominant symbol per cell along a monotone alignment), full lengths."""
    acts, labels, il, ll = fc.trained_like_case(B, T, L + 1, V, seed)
    return acts, labels, il, ll


RAGGED_LENGTHS = [(40, 20), (40, 0), (1, 0), (1, 1), (20, 20), (7, 12)]  # the last: more labels than frames


def ragged_case(seed=0):
    B, T, U, V = 6, 40, 21, 28
    rng = np.random.default_rng(seed)
    acts = rng.normal(size=(B, T, U, V)).astype(np.float32)
    labels = rng.integers(1, V, size=(B, U - 1)).astype(np.int32)
    il = np.array([t for t, _ in RAGGED_LENGTHS], np.int32)
    ll = np.array([l for _, l in RAGGED_LENGTHS], np.int32)
    return acts, labels, il, ll
