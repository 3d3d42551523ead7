"""The simple (additive joiner) transducer loss of include/rnnt_simple.h compute_rnnt_loss_simple, restated in float64 NumPy from
its contract, and the input builders the CPU and GPU tests share.  Nothing of the code under test is imported.

Per utterance: T frames, L labels, am [T, V], lm [L + 1, V]; a = am_only_scale, l = lm_only_scale, w = 1 - a - l:
    Z(t,u) = ln sum_v exp(am[t,v] + lm[u,v]),  Za(t) = ln sum_v exp(am[t,v]),  Zl(u) = ln sum_v exp(lm[u,v])
    lp(t,u,v) = w (am[t,v] + lm[u,v] - Z(t,u)) + a (am[t,v] - Za(t)) + l (lm[u,v] - Zl(u))
    standard:  alpha(0,0) = 0;  alpha(t,u) = logaddexp(alpha(t-1,u) + lpb(t-1,u), alpha(t,u-1) + lpl(t,u-1))
               ln P = alpha(T-1,L) + lpb(T-1,L);  beta(T-1,L) = lpb(T-1,L)
               beta(t,u) = logaddexp(lpb(t,u) + beta(t+1,u), lpl(t,u) + beta(t,u+1))
    modified:  alpha(t,u) = logaddexp(alpha(t-1,u) + lpb(t-1,u), alpha(t-1,u-1) + lpl(t-1,u-1));  ln P = alpha(T,L)
               beta(T,L) = 0;  beta(t,u) = logaddexp(lpb(t,u) + beta(t+1,u), lpl(t,u) + beta(t+1,u+1))
    e_b = exp(alpha + lpb + beta(blank target) - ln P),  e_l = exp(alpha + lpl + beta(label target) - ln P),  occ = e_b + e_l
    grad_am[t,v] = cs (w sum_u occ sj + a sa sum_u occ - (w + a) sum_u eps),  grad_lm[u,v] likewise over t with l and sl
No path (modified, L > T): cost +inf, everything else zero."""
import math

import numpy as np

NINF = -math.inf
TOPOLOGIES = ("standard", "modified")
SCALES = ((0.0, 0.0), (0.25, 0.0), (0.0, 0.25), (0.25, 0.25), (1.0, 0.0), (0.0, 1.0))  # (lm_only_scale, am_only_scale)


def _lae(a, b):
    if a < b:
        a, b = b, a
    if b == NINF:
        return a
    return a + math.log1p(math.exp(b - a))


def _lsm(x):
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def edge_logprobs(am, lm, y, blank, l, a):
    """am [T, V], lm [L + 1, V], y [L] -> (lsj [T, L+1, V], lsa, lsl, lpb [T, L+1], lpl [T, L+1] with -inf at u = L)."""
    am, lm = np.asarray(am, np.float64), np.asarray(lm, np.float64)
    T, L = am.shape[0], lm.shape[0] - 1
    w = 1.0 - a - l
    lsj = _lsm(am[:, None, :] + lm[None, :, :])
    lsa, lsl = _lsm(am), _lsm(lm)
    lp = w * lsj + a * lsa[:, None, :] + l * lsl[None, :, :]
    lpb = lp[:, :, blank]
    lpl = np.full((T, L + 1), NINF)
    for u in range(L):
        lpl[:, u] = lp[:, u, y[u]]
    return lsj, lsa, lsl, lpb, lpl


def lattice(lpb, lpl, topology):
    """(ln P, e_b [T, L+1], e_l [T, L+1]); zeros when there is no path."""
    T, U = lpb.shape
    L = U - 1
    al = [[NINF] * U for _ in range(T + 1)]
    be = [[NINF] * (U + 1) for _ in range(T + 1)]
    al[0][0] = 0.0
    if topology == "standard":
        for t in range(T):
            for u in range(U):
                if t > 0:
                    al[t][u] = _lae(al[t][u], al[t - 1][u] + lpb[t - 1, u])
                if u > 0:
                    al[t][u] = _lae(al[t][u], al[t][u - 1] + lpl[t, u - 1])
        ll = al[T - 1][L] + lpb[T - 1, L]
        be[T][L] = 0.0  # the end: the final blank's target
        for t in range(T - 1, -1, -1):
            for u in range(L, -1, -1):
                be[t][u] = _lae(lpb[t, u] + be[t + 1][u], lpl[t, u] + be[t][u + 1] if u < L else NINF)
    else:
        for t in range(1, T + 1):
            for u in range(U):
                al[t][u] = _lae(al[t - 1][u] + lpb[t - 1, u], al[t - 1][u - 1] + lpl[t - 1, u - 1] if u > 0 else NINF)
        ll = al[T][L]
        be[T][L] = 0.0
        for t in range(T - 1, -1, -1):
            for u in range(L, -1, -1):
                be[t][u] = _lae(lpb[t, u] + be[t + 1][u], lpl[t, u] + be[t + 1][u + 1] if u < L else NINF)
    e_b, e_l = np.zeros((T, U)), np.zeros((T, U))
    if ll == NINF:
        return ll, e_b, e_l
    for t in range(T):
        for u in range(U):
            if al[t][u] == NINF:
                continue
            x = al[t][u] + lpb[t, u] + be[t + 1][u] - ll
            e_b[t, u] = math.exp(x) if x != NINF else 0.0
            if u < L:
                x = al[t][u] + lpl[t, u] + (be[t][u + 1] if topology == "standard" else be[t + 1][u + 1]) - ll
                e_l[t, u] = math.exp(x) if x != NINF else 0.0
    return ll, e_b, e_l


def utterance(am, lm, y, blank=0, l=0.0, a=0.0, topology="standard"):
    """One utterance with exact lengths: (cost, e_b, e_l, grad_am [T, V], grad_lm [L+1, V]) in float64."""
    am, lm = np.asarray(am, np.float64), np.asarray(lm, np.float64)
    V = am.shape[1]
    L = lm.shape[0] - 1
    y = [min(max(int(v), 0), V - 1) for v in np.asarray(y)[:L]]
    w = 1.0 - a - l
    lsj, lsa, lsl, lpb, lpl = edge_logprobs(am, lm, y, blank, l, a)
    ll, e_b, e_l = lattice(lpb, lpl, topology)
    if ll == NINF:
        return np.inf, e_b, e_l, np.zeros_like(am), np.zeros_like(lm)
    occ = e_b + e_l
    eps = np.zeros_like(lsj)
    eps[:, :, blank] += e_b
    for u in range(L):
        eps[:, u, y[u]] += e_l[:, u]
    sj = np.exp(lsj)
    g_am = w * np.einsum("tu,tuv->tv", occ, sj) + a * np.exp(lsa) * occ.sum(1)[:, None] - (w + a) * eps.sum(1)
    g_lm = w * np.einsum("tu,tuv->uv", occ, sj) + l * np.exp(lsl) * occ.sum(0)[:, None] - (w + l) * eps.sum(0)
    return -ll, e_b, e_l, g_am, g_lm


def loss_and_grad(am, lm, labels, il, ll, blank=0, l=0.0, a=0.0, topology="standard", cost_scale=None):
    """Batched, ragged: dict(costs [B], occ [B, T, U], e_b, e_l, g_am [B, T, V], g_lm [B, U, V]); padding is zero; the gradients
    carry cost_scale.  Only the live rows am[b, :T_b] and lm[b, :L_b + 1] are touched."""
    am, lm = np.asarray(am), np.asarray(lm)
    B, T, V = am.shape
    U = lm.shape[1]
    cs = np.ones(B) if cost_scale is None else np.broadcast_to(np.asarray(cost_scale, np.float64), (B,))
    out = dict(costs=np.zeros(B), e_b=np.zeros((B, T, U)), e_l=np.zeros((B, T, U)), g_am=np.zeros((B, T, V)), g_lm=np.zeros((B, U, V)))
    for b in range(B):
        Tb, Lb = int(il[b]), int(ll[b])
        c, e_b, e_l, ga, gl = utterance(am[b, :Tb], lm[b, :Lb + 1], labels[b], blank, l, a, topology)
        out["costs"][b] = c
        out["e_b"][b, :Tb, :Lb + 1], out["e_l"][b, :Tb, :Lb + 1] = e_b, e_l
        out["g_am"][b, :Tb], out["g_lm"][b, :Lb + 1] = cs[b] * ga, cs[b] * gl
    out["occ"] = out["e_b"] + out["e_l"]
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------
def poison(am, lm, il, ll):
    """NaN in every row the op must not read (in place): am[b, t >= T_b], lm[b, u > L_b]."""
    for b in range(am.shape[0]):
        am[b, int(il[b]):] = np.nan
        lm[b, int(ll[b]) + 1:] = np.nan
    return am, lm


def case(B, T, U, V, seed, sigma=1.0, blank=0, ragged=True, full_first=True):
    """(am [B, T, V], lm [B, U, V] float32 with NaN in the unread rows, labels [B, max(U - 1, 1)] without the blank, il, ll)."""
    rng = np.random.default_rng(seed)
    am = (rng.normal(size=(B, T, V)) * sigma).astype(np.float32)
    lm = (rng.normal(size=(B, U, V)) * sigma).astype(np.float32)
    labels = rng.integers(0, V - 1, size=(B, max(U - 1, 1))).astype(np.int32)
    labels += labels >= blank
    il, ll = np.full(B, T, np.int32), np.full(B, U - 1, np.int32)
    if ragged and B > 1:
        il[:] = rng.integers((T + 1) // 2, T + 1, size=B)
        ll[:] = rng.integers((U - 1) // 2, U, size=B)
        if full_first:
            il[0], ll[0] = T, U - 1
    poison(am, lm, il, ll)
    return am, lm, labels, il, ll


def trained_like_case(B, T, U, V, seed):
    """One dominant symbol along a monotone alignment, as far as an additive joiner can say it: lm[u] prefers y_u (+3), am[t]
    prefers the blank (+3) except on the frames where the straight line from (0, 0) to (T_b, L_b) emits (-3 on the blank);
    0.5 x N(0,1) underneath."""
    am, lm, labels, il, ll = case(B, T, U, V, seed, sigma=0.5)
    for b in range(B):
        Tb, Lb = int(il[b]), int(ll[b])
        for u in range(Lb):
            lm[b, u, labels[b, u]] += 3.0
        emit = {int((k + 0.5) * Tb / max(Lb, 1)) for k in range(Lb)}
        for t in range(Tb):
            am[b, t, 0] += -3.0 if t in emit else 3.0
    return am, lm, labels, il, ll
