"""FastEmit (include/rnnt.h compute_rnnt_loss_fastemit) restated in float64 NumPy on the oracle's own lattice code, the same
for the fused joints (FastEmit's dlogits pushed through oracle.rnnt_oracle.joint_backward), and the input builders the CPU and
GPU tests share.

Definition, per utterance (lp = log_softmax(x), alpha / beta / ln P from oracle.rnnt_oracle):
    e_b(t,u) = exp(alpha + lp[blank] + beta(t+1,u) - ln P)   t < T-1;   exp(alpha + lp[blank] - ln P) at (T-1, U-1);   else 0
    e_l(t,u) = exp(alpha + lp[y_u]   + beta(t,u+1) - ln P)   u < U-1;   else 0
    occ      = e_b + e_l
    grads[t,u,v] = cs ((occ + lambda e_l) softmax(x)[v] - [v == blank] e_b - [v == y_u] (1 + lambda) e_l)
The cost stays -ln P."""
import numpy as np

from oracle import rnnt_oracle as orc


def utterance(x, labels, lam, blank=0):
    """One utterance with exact lengths: x [T, U, V] logits -> (cost, grads [T, U, V]) in float64."""
    x = np.asarray(x, np.float64)
    T, U, V = x.shape
    lp = orc.log_softmax(x)
    lpb, lpl = orc._gather(lp, labels, blank)
    a, ll = orc.alphas(lpb, lpl)
    b, _ = orc.betas(lpb, lpl)
    e_b = np.zeros((T, U))
    e_b[: T - 1] = np.exp(a[: T - 1] + lpb[: T - 1] + b[1:] - ll)
    e_b[T - 1, U - 1] = np.exp(a[T - 1, U - 1] + lpb[T - 1, U - 1] - ll)
    e_l = np.zeros((T, U))
    if U > 1:
        e_l[:, : U - 1] = np.exp(a[:, : U - 1] + lpl + b[:, 1:] - ll)
    occ = e_b + e_l
    g = (occ + lam * e_l)[:, :, None] * np.exp(lp)
    g[:, :, blank] -= e_b
    if U > 1:
        idx = np.asarray(labels[: U - 1], np.int64)
        np.subtract.at(g, (np.arange(T)[:, None], np.arange(U - 1)[None, :], idx[None, :]), (1.0 + lam) * e_l[:, : U - 1])
    return -ll, g


def loss_and_grad(acts, labels, il, ll, lam, cost_scale=None, blank=0):
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


def joint_loss_and_grads(enc, pred, W1, b1, W2, b2, labels, il, ll, lam, cost_scale=None, blank=0):
    """The joint network (unrounded float64) + FastEmit: costs and the six gradients (+ d_a / d_c: the projections' gradients)."""
    y, h = orc.joint_forward(enc, pred, W1, b1, W2, b2)
    costs, g = loss_and_grad(y, labels, il, ll, lam, cost_scale, blank)
    out = orc.joint_backward(g, enc, pred, W1, b1, W2, b2, h)
    out["costs"] = costs
    return out


GRAD_KEYS = ("d_enc", "d_pred", "dW1", "db1", "dW2", "db2")


# ---- inputs -------------------------------------------------------------------------------------------------------------
def ragged_lengths(rng, B, T, U):
    il = rng.integers((T + 1) // 2, T + 1, size=B).astype(np.int32)
    ll = rng.integers(U // 2, U, size=B).astype(np.int32)
    il[0], ll[0] = T, U - 1
    return il, ll


def op_case(B, T, U, V, seed, sigma=1.0):
    rng = np.random.default_rng(seed)
    acts = (rng.normal(size=(B, T, U, V)) * sigma).astype(np.float32)
    labels = rng.integers(1, V, size=(B, max(U - 1, 1))).astype(np.int32)
    il, ll = ragged_lengths(rng, B, T, U)
    return acts, labels, il, ll


def trained_like_case(B, T, U, V, seed):
    """One dominant symbol per cell along a monotone alignment: the label where the straight line from (0, 0) to (T, U) says
    'emit', the blank elsewhere (+6 on top of 0.5 x N(0,1))."""
    rng = np.random.default_rng(seed)
    acts, labels, il, ll = op_case(B, T, U, V, seed, sigma=0.5)
    for b in range(B):
        Tb, Ub = int(il[b]), int(ll[b]) + 1
        for t in range(Tb):
            for u in range(Ub):
                emit = u < Ub - 1 and (u + 1) * Tb <= (t + 1) * (Ub - 1)
                acts[b, t, u, labels[b, u] if emit else 0] += 6.0
    return acts, labels, il, ll


def hand_back_case():
    """The smallest input with which tests/test_lin_gpu.py forces a hand-back (test_tiny_edge_probabilities): B2 T12 U6 V8, full
    lengths, utterance 0's labels at a probability below 2^-100."""
    rng = np.random.default_rng(3)
    B, T, U, V = 2, 12, 6, 8
    acts = rng.normal(size=(B, T, U, V)).astype(np.float32)
    labels = rng.integers(1, V, size=(B, U - 1)).astype(np.int32)
    il, ll = np.full(B, T, np.int32), np.full(B, U - 1, np.int32)
    for u in range(5):
        acts[0, :, u, labels[0, u]] = -90.0
    return acts, labels, il, ll


def joint_case(B, T, U, H, J, V, seed, f16_recipe=False):
    """N(0,1) encoder / prediction outputs; glorot weights (x 3 on W2 with tests/test_joint_f16_gpu.py's recipe), ragged lengths."""
    rng = np.random.default_rng(seed)
    enc = rng.normal(size=(B, T, H)).astype(np.float32)
    pred = rng.normal(size=(B, U, H)).astype(np.float32)
    lim1, lim2 = np.sqrt(6.0 / (H + J)), np.sqrt(6.0 / (J + V))
    W1 = rng.uniform(-lim1, lim1, size=(H, J)).astype(np.float32)
    b1 = (0.1 * rng.normal(size=J)).astype(np.float32)
    W2 = rng.uniform(-lim2, lim2, size=(J, V)).astype(np.float32) * (3.0 if f16_recipe else 1.0)
    b2 = (0.1 * rng.normal(size=V)).astype(np.float32)
    labels = rng.integers(1, V, size=(B, U - 1)).astype(np.int32)
    il, ll = ragged_lengths(rng, B, T, U)
    return enc, pred, W1, b1, W2, b2, labels, il, ll


def proj_case(B, T, U, J, V, seed):
    """N(0,1) projections for compute_rnnt_joint_loss_*: as a joint network with W1 = I (H = J), b1 = 0."""
    enc, pred, _, _, W2, b2, labels, il, ll = joint_case(B, T, U, J, J, V, seed)
    return enc, pred, np.eye(J, dtype=np.float32), np.zeros(J, np.float32), W2, b2, labels, il, ll
