"""The token-and-duration (TDT) transducer lattice of include/rnnt_tdt.h compute_rnnt_loss_tdt, restated in float64 NumPy from its
equations, and the input builders the CPU and GPU tests share.

Per utterance, T frames, L labels, x [T, L+1, V + D]: lp = log_softmax(x[..., :V]), ld = log_softmax(x[..., V:]); nodes (t, u),
0 <= t < T, 0 <= u <= L, and the terminal (T, L).  From (t, u), for each i with d = durations[i]:
    blank edge to (t+d, u),    wb_i = lp(t,u,blank) - sigma + ld(t,u,i),  iff d > 0 and (t+d < T, or t+d == T and u == L)
    label edge to (t+d, u+1),  wl_i = lp(t,u,y_u)  - sigma + ld(t,u,i),  iff u < L and t+d < T
    alpha(0,0) = 0, alpha(node) = logsumexp over incoming edges;  ln P = alpha(T,L), cost = -ln P
    beta(T,L) = 0,  beta(t,u)  = logsumexp over outgoing edges of w + beta(target)
    e(edge) = exp(alpha(t,u) + w + beta(target) - ln P); g_b / g_l = the sums over blank / label edges, g_i over both edges of
    duration i, m = g_b + g_l:
    grads[t,u,v]     = cs (m softmax(x[t,u,:V])[v] - [v == blank] g_b - [u < L and v == y_u] g_l)
    grads[t,u,V + i] = cs (m softmax(x[t,u,V:])[i] - g_i)
No path: cost +inf, gradients zero."""
import numpy as np


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def _lse(terms):
    terms = [v for v in terms if v != -np.inf]
    if not terms:
        return -np.inf
    m = max(terms)
    return m + np.log(sum(np.exp(v - m) for v in terms))


def out_edges(t, u, T, L, durations):
    """The edges out of cell (t, u): [(i, is_label, (t', u'))] in the order of i, blank before label."""
    out = []
    for i, d in enumerate(durations):
        if d > 0 and (t + d < T or (t + d == T and u == L)):
            out.append((i, False, (t + d, u)))
        if u < L and t + d < T:
            out.append((i, True, (t + d, u + 1)))
    return out


def weights(x, labels, durations, blank=0, sigma=0.0):
    """x [T, L+1, V + D] -> (lp, ld, wb [T, L+1, D], wl [T, L+1, D], y); wl of column L is unused.  Labels are clamped into [0, V)."""
    x = np.asarray(x, np.float64)
    T, U, R = x.shape
    V = R - len(durations)
    lp, ld = log_softmax(x[..., :V]), log_softmax(x[..., V:])
    y = np.clip(np.asarray(labels[: U - 1], np.int64), 0, V - 1)
    wb = (lp[:, :, blank] - sigma)[:, :, None] + ld
    wl = np.zeros_like(wb)
    if U > 1:
        wl[:, : U - 1] = (lp[:, np.arange(U - 1), y] - sigma)[:, :, None] + ld[:, : U - 1]
    return lp, ld, wb, wl, y


def alphas(wb, wl, durations):
    """alpha [T + 1, L + 1] (row T: the terminal's column L alone), by pushing every node's mass along its edges in (t, u) order."""
    T, U, _ = wb.shape
    L = U - 1
    inc = [[[] for _ in range(U)] for _ in range(T + 1)]
    a = np.full((T + 1, U), -np.inf)
    for t in range(T):
        for u in range(U):  # d = 0 label edges go to (t, u + 1): row-major order visits every source before its targets
            a[t, u] = 0.0 if (t, u) == (0, 0) else _lse(inc[t][u])
            for i, label, (t2, u2) in out_edges(t, u, T, L, durations):
                inc[t2][u2].append(a[t, u] + (wl if label else wb)[t, u, i])
    a[T, L] = _lse(inc[T][L])
    return a


def betas(wb, wl, durations):
    T, U, _ = wb.shape
    L = U - 1
    b = np.full((T + 1, U), -np.inf)
    b[T, L] = 0.0
    for t in range(T - 1, -1, -1):
        for u in range(L, -1, -1):
            b[t, u] = _lse([(wl if label else wb)[t, u, i] + b[t2, u2] for i, label, (t2, u2) in out_edges(t, u, T, L, durations)])
    return b


def utterance(x, labels, durations, blank=0, sigma=0.0):
    """One utterance with exact lengths: x [T, L+1, V + D] logits -> (cost, grads [T, L+1, V + D]) in float64."""
    x = np.asarray(x, np.float64)
    T, U, R = x.shape
    D = len(durations)
    V, L = R - D, U - 1
    lp, ld, wb, wl, y = weights(x, labels, durations, blank, sigma)
    a, b = alphas(wb, wl, durations), betas(wb, wl, durations)
    lnP = a[T, L]
    g = np.zeros((T, U, R))
    if lnP == -np.inf:
        return np.inf, g
    for t in range(T):
        for u in range(U):
            if a[t, u] == -np.inf:
                continue
            gb = gl = 0.0
            gi = np.zeros(D)
            for i, label, (t2, u2) in out_edges(t, u, T, L, durations):
                e = np.exp(a[t, u] + (wl if label else wb)[t, u, i] + b[t2, u2] - lnP)
                gi[i] += e
                if label:
                    gl += e
                else:
                    gb += e
            m = gb + gl
            if m == 0.0:
                continue
            g[t, u, :V] = m * np.exp(lp[t, u])
            g[t, u, blank] -= gb
            if u < L:
                g[t, u, y[u]] -= gl
            g[t, u, V:] = m * np.exp(ld[t, u]) - gi
    return -lnP, g


def loss_and_grad(acts, labels, il, ll, durations, blank=0, sigma=0.0, cost_scale=None):
    """Batched, ragged: (costs [B], grads [B, T, U, V + D]); padded cells are zeros; grads carry cost_scale."""
    acts = np.asarray(acts)
    B, T, U, R = acts.shape
    costs, grads = np.zeros(B), np.zeros((B, T, U, R))
    cs = np.ones(B) if cost_scale is None else np.broadcast_to(np.asarray(cost_scale, np.float64), (B,))
    for i in range(B):
        Tb, Ub = int(il[i]), int(ll[i]) + 1
        c, g = utterance(acts[i, :Tb, :Ub], np.asarray(labels[i])[: Ub - 1], durations, blank, sigma)
        costs[i] = c
        grads[i, :Tb, :Ub] = cs[i] * g
    return costs, grads


def crossed_mask(acts, labels, il, ll, durations, blank=0):
    """bool [B, T, U]: True on the live cells a path crosses (alpha finite and some existing edge's target has a finite beta)."""
    acts = np.asarray(acts)
    B, T, U, _ = acts.shape
    mask = np.zeros((B, T, U), bool)
    for i in range(B):
        Tb, Lb = int(il[i]), int(ll[i])
        _, _, wb, wl, _ = weights(acts[i, :Tb, : Lb + 1], np.asarray(labels[i])[:Lb], durations, blank)
        a, b = alphas(wb, wl, durations), betas(wb, wl, durations)
        if a[Tb, Lb] == -np.inf:
            continue
        for t in range(Tb):
            for u in range(Lb + 1):
                mask[i, t, u] = a[t, u] > -np.inf and any(b[n] > -np.inf for _, _, n in out_edges(t, u, Tb, Lb, durations))
    return mask


def brute_force_cost(x, labels, durations, blank=0, sigma=0.0):
    """-ln of the sum over every path from (0, 0) to the terminal, enumerated edge by edge."""
    x = np.asarray(x, np.float64)
    T, U, _ = x.shape
    L = U - 1
    _, _, wb, wl, _ = weights(x, labels, durations, blank, sigma)
    totals = []

    def walk(t, u, s):
        if (t, u) == (T, L):
            totals.append(s)
            return
        for i, label, (t2, u2) in out_edges(t, u, T, L, durations):
            walk(t2, u2, s + (wl if label else wb)[t, u, i])

    walk(0, 0, 0.0)
    return -_lse(totals) if totals else np.inf


# ---- inputs -------------------------------------------------------------------------------------------------------------
def full_case(B, T, L, V, D, seed, scale=1.0, blank=0):
    """Full lengths; labels avoid the blank.  acts [B, T, L + 1, V + D]."""
    rng = np.random.default_rng(seed)
    acts = (rng.normal(size=(B, T, L + 1, V + D)) * scale).astype(np.float32)
    labels = rng.integers(0, V - 1, size=(B, max(L, 1))).astype(np.int32)
    labels += labels >= blank
    return acts, labels, np.full(B, T, np.int32), np.full(B, L, np.int32)


def ragged_case(lengths, V, D, seed, scale=1.0, blank=0):
    """One utterance per (T_b, L_b) of `lengths` in a batch of maxT = max T_b, maxU = max L_b + 1."""
    T, L = max(t for t, _ in lengths), max(l for _, l in lengths)
    acts, labels, il, ll = full_case(len(lengths), T, L, V, D, seed, scale, blank)
    il[:] = [t for t, _ in lengths]
    ll[:] = [l for _, l in lengths]
    return acts, labels, il, ll


def trained_like_case(B, T, L, V, durations, seed, peak=6.0, blank=0):
    """Peaked posteriors along one feasible path per utterance: every cell of the path has its token (the next label or the blank)
    and its duration `peak` above N(0,1) noise, as a trained TDT model's joint has; full lengths."""
    acts, labels, il, ll = full_case(B, T, L, V, len(durations), seed, blank=blank)
    rng = np.random.default_rng(seed + 1)
    pos = [i for i, d in enumerate(durations) if d > 0]
    for b in range(B):
        emit = np.sort(rng.choice(T, size=L, replace=True)) if L else np.zeros(0, int)  # the frame each label is emitted on
        t = u = 0
        while t < T:
            if u < L and emit[u] <= t:
                i = 0 if durations[0] == 0 and rng.random() < 0.5 else pos[0]
                if t + durations[i] >= T:  # a label edge never lands on T
                    i = 0 if durations[0] == 0 else None
                if i is not None:
                    acts[b, t, u, labels[b, u]] += peak
                    acts[b, t, u, V + i] += peak
                    t, u = t + durations[i], u + 1
                    continue
            fits = [i for i in pos if t + durations[i] <= T and (t + durations[i] < T or u == L)] or pos[:1]
            i = fits[int(rng.integers(len(fits)))]
            acts[b, t, u, blank] += peak
            acts[b, t, u, V + i] += peak
            t += durations[i]
    return acts, labels, il, ll
