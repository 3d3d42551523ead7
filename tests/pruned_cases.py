"""The pruned transducer loss of include/rnnt_pruned.h compute_rnnt_loss_pruned, restated in float64 from its contract, and the
input builders the CPU and GPU tests share.  Nothing of the code under test is imported.

Per utterance: T frames, L labels, a band of S slots per frame; slot (t, s) is lattice cell (t, u), u = sb[t] + s, PRESENT iff
0 <= t < T and 0 <= u <= L.  Absent cells have no edges and zero gradients; their logits are never read (the tests put NaN there).
    standard:  alpha(0,0) = 0;  alpha(t,u) = logaddexp(alpha(t-1,u) + lpb(t-1,u), alpha(t,u-1) + lpl(t,u-1))
               ln P = alpha(T-1,L) + lpb(T-1,L);  beta(T-1,L) = lpb(T-1,L)
               beta(t,u) = logaddexp(lpb(t,u) + beta(t+1,u), lpl(t,u) + beta(t,u+1))
    modified:  alpha(t,u) = logaddexp(alpha(t-1,u) + lpb(t-1,u), alpha(t-1,u-1) + lpl(t-1,u-1));  ln P = alpha(T,L)
               beta(T,L) = 0;  beta(t,u) = logaddexp(lpb(t,u) + beta(t+1,u), lpl(t,u) + beta(t+1,u+1))
    e_b = exp(alpha + lpb + beta(blank target) - ln P),  e_l = exp(alpha + lpl + beta(label target) - ln P)
    grads[t,s,v] = cs ((e_b + e_l + lambda e_l) softmax[v] - [v == blank] e_b - [v == y_u] (1 + lambda) e_l)
A term whose source or target cell is absent is -inf.  No path: cost +inf, gradients zero."""
import math

import numpy as np

from tests import fastemit_cases as fc

NINF = -math.inf
TOPOLOGIES = ("standard", "modified")


def _lae(a, b):
    if a < b:
        a, b = b, a
    if b == NINF:
        return a
    return a + math.log1p(math.exp(b - a))


def edges(x, sb, labels, T, L, blank=0):
    """x [maxT, S, V], sb [maxT] -> dict: present [T, S] bool, u [T, S] (Python ints), lp [T, S, V] (zeros where absent),
    lpb / lpl [T][S] lists (-inf where absent / where there is no label edge), y [T, S] (the label of the cell, -1 without)."""
    x = np.asarray(x)
    S, V = x.shape[1], x.shape[2]
    u = [[int(sb[t]) + s for s in range(S)] for t in range(T)]
    present = np.array([[0 <= u[t][s] <= L for s in range(S)] for t in range(T)], bool).reshape(T, S)
    xs = np.where(present[:, :, None], np.asarray(x[:T], np.float64), 0.0)  # absent logits are never read
    m = xs.max(axis=-1, keepdims=True)
    lp = (xs - m - np.log(np.exp(xs - m).sum(axis=-1, keepdims=True))) * present[:, :, None]
    y = -np.ones((T, S), np.int64)
    lpb = [[NINF] * S for _ in range(T)]
    lpl = [[NINF] * S for _ in range(T)]
    for t, s in zip(*np.nonzero(present)):
        lpb[t][s] = float(lp[t, s, blank])
        if u[t][s] < L:
            y[t, s] = min(max(int(labels[u[t][s]]), 0), V - 1)
            lpl[t][s] = float(lp[t, s, y[t, s]])
    return dict(present=present, u=u, lp=lp, lpb=lpb, lpl=lpl, y=y, T=T, L=L, S=S)


def _slot(e, t, u):
    """The slot of lattice cell (t, u) in row t, or None when the cell is absent."""
    if not 0 <= t < e["T"] or not 0 <= u <= e["L"]:
        return None
    s = u - e["u"][t][0]
    return s if 0 <= s < e["S"] else None


def alphas(e, topology):
    """(alpha [T][S] lists with -inf on absent cells, ln P)."""
    T, L, S = e["T"], e["L"], e["S"]
    a = [[NINF] * S for _ in range(T)]
    for t in range(T):
        for s in range(S):
            if not e["present"][t, s]:
                continue
            u = e["u"][t][s]
            v = 0.0 if (t == 0 and u == 0) else NINF
            q = _slot(e, t - 1, u)
            if q is not None:
                v = _lae(v, a[t - 1][q] + e["lpb"][t - 1][q])
            q = _slot(e, t, u - 1) if topology == "standard" else _slot(e, t - 1, u - 1)
            if q is not None:
                tq = t if topology == "standard" else t - 1
                v = _lae(v, a[tq][q] + e["lpl"][tq][q])
            a[t][s] = v
    ll = NINF
    q = _slot(e, T - 1, L)
    if q is not None:
        ll = a[T - 1][q] + e["lpb"][T - 1][q]
    if topology == "modified":
        q = _slot(e, T - 1, L - 1)
        if q is not None:
            ll = _lae(ll, a[T - 1][q] + e["lpl"][T - 1][q])
    return a, ll


def betas(e, topology):
    """(blank term, label term) [T][S]: lpb + beta(blank target) and lpl + beta(label target), -inf where the edge or its target
    is absent; beta = logaddexp of the two."""
    T, L, S = e["T"], e["L"], e["S"]
    beta = [[NINF] * S for _ in range(T)]
    tb = [[NINF] * S for _ in range(T)]
    tl = [[NINF] * S for _ in range(T)]
    for t in range(T - 1, -1, -1):
        for s in range(S - 1, -1, -1):
            if not e["present"][t, s]:
                continue
            u = e["u"][t][s]
            if t == T - 1:
                nb = 0.0 if u == L else NINF                                   # the final blank / the end node (T, L)
                nl = 0.0 if (topology == "modified" and u + 1 == L) else NINF
            else:
                q = _slot(e, t + 1, u)
                nb = beta[t + 1][q] if q is not None else NINF
                nl = NINF
                if topology == "modified":
                    q = _slot(e, t + 1, u + 1)
                    nl = beta[t + 1][q] if q is not None else NINF
            if topology == "standard":
                q = _slot(e, t, u + 1)
                nl = beta[t][q] if q is not None else NINF
            tb[t][s] = e["lpb"][t][s] + nb
            tl[t][s] = e["lpl"][t][s] + nl if u < L else NINF
            beta[t][s] = _lae(tb[t][s], tl[t][s])
    return tb, tl


def occupancies(e, topology):
    """(ln P, e_b [T, S], e_l [T, S]); zeros when there is no path."""
    T, S = e["T"], e["S"]
    a, ll = alphas(e, topology)
    e_b, e_l = np.zeros((T, S)), np.zeros((T, S))
    if ll == NINF:
        return ll, e_b, e_l
    tb, tl = betas(e, topology)
    for t in range(T):
        for s in range(S):
            if a[t][s] == NINF:
                continue
            if tb[t][s] != NINF:
                e_b[t, s] = math.exp(a[t][s] + tb[t][s] - ll)
            if tl[t][s] != NINF:
                e_l[t, s] = math.exp(a[t][s] + tl[t][s] - ll)
    return ll, e_b, e_l


def utterance(x, sb, labels, T, L, lam=0.0, blank=0, topology="standard"):
    """One utterance: x [maxT, S, V], sb [maxT] -> (cost, grads [maxT, S, V]) in float64; absent cells are zeros."""
    x = np.asarray(x)
    e = edges(x, sb, labels, T, L, blank)
    ll, e_b, e_l = occupancies(e, topology)
    g = np.zeros(x.shape, np.float64)
    if ll == NINF:
        return np.inf, g
    gt = (e_b + (1.0 + lam) * e_l)[:, :, None] * np.exp(e["lp"]) * e["present"][:, :, None]
    gt[:, :, blank] -= e_b
    tt, ss = np.nonzero(e["y"] >= 0)
    np.subtract.at(gt, (tt, ss, e["y"][tt, ss]), (1.0 + lam) * e_l[tt, ss])
    g[:T] = gt
    return -ll, g


def loss_and_grad(acts, s_begin, labels, il, ll, lam=0.0, cost_scale=None, blank=0, topology="standard"):
    """Batched, ragged: (costs [B], grads [B, T, S, V]); grads carry cost_scale."""
    acts = np.asarray(acts)
    B = acts.shape[0]
    costs, grads = np.zeros(B), np.zeros(acts.shape, np.float64)
    cs = np.ones(B) if cost_scale is None else np.broadcast_to(np.asarray(cost_scale, np.float64), (B,))
    for i in range(B):
        c, g = utterance(acts[i], s_begin[i], labels[i], int(il[i]), int(ll[i]), lam, blank, topology)
        costs[i] = c
        grads[i] = cs[i] * g
    return costs, grads


def present_mask(s_begin, il, ll, S):
    """bool [B, T, S]: the present cells."""
    sb = np.asarray(s_begin, np.int64)
    B, T = sb.shape
    u = sb[:, :, None] + np.arange(S)[None, None, :]
    t = np.arange(T)[None, :, None]
    return (t < np.asarray(il)[:, None, None]) & (u >= 0) & (u <= np.asarray(ll, np.int64)[:, None, None])


def full_occupancy(acts, labels, il, ll, blank=0, topology="standard"):
    """e_b + e_l per cell of the FULL lattice, [B, T, U]: the restatement with sb = 0 and S = U (what a first pass would give)."""
    acts = np.asarray(acts)
    B, T, U, _ = acts.shape
    occ = np.zeros((B, T, U))
    for i in range(B):
        Tb, Lb = int(il[i]), int(ll[i])
        e = edges(acts[i], np.zeros(T, np.int64), labels[i], Tb, Lb, blank)
        _, e_b, e_l = occupancies(e, topology)
        occ[i, :Tb] = e_b + e_l
    return occ


def brute_force_cost(x, sb, labels, T, L, blank=0, topology="standard"):
    """-ln of the sum over every path of the banded lattice, one path at a time (tiny lattices only)."""
    e = edges(x, sb, labels, T, L, blank)
    terms = []

    def walk(t, u, s):
        if topology == "modified" and t == T:
            if u == L:
                terms.append(s)
            return
        q = _slot(e, t, u)
        if q is None:
            return
        if topology == "standard":
            if t == T - 1 and u == L:
                terms.append(s + e["lpb"][t][q])
                return
            walk(t + 1, u, s + e["lpb"][t][q])
            if u < L:
                walk(t, u + 1, s + e["lpl"][t][q])
        else:
            walk(t + 1, u, s + e["lpb"][t][q])
            if u < L:
                walk(t + 1, u + 1, s + e["lpl"][t][q])

    walk(0, 0, 0.0)
    if not terms:
        return np.inf
    m = max(terms)
    return -(m + math.log(sum(math.exp(v - m) for v in terms)))


# ---- inputs -------------------------------------------------------------------------------------------------------------
def gather_band(full, s_begin, S, fill=np.nan):
    """full [B, T, U, V] -> the band's tensor [B, T, S, V] float32; every slot outside [0, U) holds `fill`."""
    full = np.asarray(full)
    B, T, U, V = full.shape
    out = np.full((B, T, S, V), fill, np.float32)
    u = np.asarray(s_begin, np.int64)[:, :, None] + np.arange(S)[None, None, :]
    ok = (u >= 0) & (u < U)
    bb, tt, ss = np.nonzero(ok)
    out[bb, tt, ss] = full[bb, tt, u[bb, tt, ss]]
    return out


def poison_absent(acts, s_begin, il, ll):
    """NaN logits in every absent cell (in place); returns acts."""
    acts[~present_mask(s_begin, il, ll, acts.shape[2])] = np.nan
    return acts


def staircase_ranges(rng, B, T, S, il, ll, steps=None):
    """Monotone band positions from (0, 0) to the end with steps drawn from `steps` (default: 0, 1 and S - 1), int32 [B, T]."""
    steps = [0, 1, max(S - 1, 0)] if steps is None else steps
    sb = np.zeros((B, T), np.int32)
    for b in range(B):
        Tb, hi = int(il[b]), max(0, int(ll[b]) + 1 - S)
        v = 0
        for t in range(1, T):
            left = Tb - 1 - t  # frames after this one
            v = min(v + int(rng.choice(steps)), hi)
            if t < Tb and hi - v > left * max(S - 1, 0):  # keep the end reachable
                v = hi - left * max(S - 1, 0)
            sb[b, t] = v
        if Tb >= 1 and S >= 1 and Tb > 1:
            sb[b, Tb - 1:] = hi
    return sb


def band_case(B, T, L, S, V, seed, sigma=1.0, blank=0, ragged=True, steps=None):
    """A random banded case: (acts [B, T, S, V] with NaN in absent cells, s_begin, labels [B, L], il, ll)."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, V - 1, size=(B, max(L, 1))).astype(np.int32)
    labels += labels >= blank
    il, ll = np.full(B, T, np.int32), np.full(B, L, np.int32)
    if ragged and B > 1:
        il[1:] = rng.integers((T + 1) // 2, T + 1, size=B - 1)
        ll[1:] = rng.integers(L // 2, L + 1, size=B - 1)
    sb = staircase_ranges(rng, B, T, S, il, ll, steps)
    acts = (rng.normal(size=(B, T, S, V)) * sigma).astype(np.float32)
    return poison_absent(acts, sb, il, ll), sb, labels, il, ll


def trained_like_case(B, T, L, V, seed):
    """tests/fastemit_cases.trained_like_case on the full lattice [B, T, L + 1, V] (one dominant symbol per cell along a monotone
    alignment), ragged lengths."""
    return fc.trained_like_case(B, T, L + 1, V, seed)
