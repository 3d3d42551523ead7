"""The CTC rule of include/rnnt_ctc.h restated in float64 NumPy from its equations, a brute-force enumerator for tiny cases, and the
input builders and case tables the CPU and GPU tests share.

Per utterance, T frames, L labels, lp = log_softmax(x), states s = 0 ... 2L with z_s = blank (even s) or y_{(s-1)/2} (odd s):
    alpha(0,0) = lp(0,blank), alpha(0,1) = lp(0,y_0), else -inf
    alpha(t,s) = lp(t,z_s) + logsumexp(alpha(t-1,s), alpha(t-1,s-1), alpha(t-1,s-2) [s odd, s >= 3, z_s != z_{s-2}])
    ln P = logaddexp(alpha(T-1,2L), alpha(T-1,2L-1)),  cost = -ln P;  beta mirrored from the last frame
    occ = exp(alpha + beta - lp(z_s) - ln P),  grads[t,v] = cs (softmax(x)[t,v] - sum_{s: z_s = v} occ(t,s))
T < L + (adjacent equal labels): no path -- cost +inf, gradients zero."""
import itertools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def _lse(*xs):
    x = np.stack(xs)
    m = x.max(axis=0)
    ms = np.where(np.isinf(m), 0.0, m)
    with np.errstate(divide="ignore"):
        return np.where(m == -np.inf, m, ms + np.log(np.exp(x - ms).sum(axis=0)))


def _up(a, n):
    """a moved n states up, -inf moved in."""
    return np.concatenate([np.full(n, -np.inf), a])[: a.size]


def _down(a, n):
    return np.concatenate([a, np.full(n, -np.inf)])[n:]


def min_frames(y):
    """The fewest frames with a path: L + the number of adjacent equal labels."""
    y = np.asarray(y)
    return int(y.size + (y[1:] == y[:-1]).sum())


def utterance(x, y, blank=0):
    """One utterance with exact lengths: x [T, V] logits, y [L] labels -> (cost, grads [T, V]) in float64."""
    x = np.asarray(x, np.float64)
    T, V = x.shape
    y = np.clip(np.asarray(y, np.int64), 0, V - 1)
    L = y.size
    S = 2 * L + 1
    lp = log_softmax(x)
    z = np.full(S, blank, np.int64)
    z[1::2] = y
    skip = np.zeros(S, bool)  # s may be entered from s - 2
    skip[3::2] = y[1:] != y[:-1]
    skip_out = np.concatenate([skip, [False, False]])[2:]  # s may be left for s + 2
    e = lp[:, z]
    alpha = np.full((T, S), -np.inf)
    alpha[0, : min(S, 2)] = e[0, : min(S, 2)]
    for t in range(1, T):
        a = alpha[t - 1]
        alpha[t] = e[t] + _lse(a, _up(a, 1), np.where(skip, _up(a, 2), -np.inf))
    beta = np.full((T, S), -np.inf)
    beta[T - 1, max(S - 2, 0):] = e[T - 1, max(S - 2, 0):]
    for t in range(T - 2, -1, -1):
        b = beta[t + 1]
        beta[t] = e[t] + _lse(b, _down(b, 1), np.where(skip_out, _down(b, 2), -np.inf))
    lnP = float(_lse(alpha[T - 1, S - 1], alpha[T - 1, S - 2])) if L else float(alpha[T - 1, 0])
    g = np.zeros((T, V))
    if lnP == -np.inf:
        return np.inf, g
    occ = np.exp(alpha + beta - e - lnP)
    g = np.exp(lp)
    for v in np.unique(z):  # (few symbols per utterance; the sum over a symbol's states)
        g[:, v] -= occ[:, z == v].sum(axis=1)
    return -lnP, g


def loss_and_grad(acts, labels, il, ll, scale=None, blank=0):
    """A batch: acts [B, T, V], labels [B, Lmax] -> (costs [B], grads [B, T, V]); padded frames are exact zeros."""
    B = acts.shape[0]
    costs, grads = np.zeros(B), np.zeros(acts.shape, np.float64)
    cs = np.ones(B) if scale is None else np.broadcast_to(np.asarray(scale, np.float64), (B,))
    for b in range(B):
        Tb, Lb = int(il[b]), int(ll[b])
        costs[b], g = utterance(acts[b, :Tb], labels[b, :Lb], blank)
        grads[b, :Tb] = cs[b] * g
    return costs, grads


def torch_ctc(acts, labels, il, ll, blank=0, scale=None):
    """torch.nn.functional.ctc_loss in float64 on the CPU: (costs [B], d sum(scale * costs) / d acts [B, T, V]); an infeasible
    utterance gets zero gradients, by the rule."""
    import torch

    x = torch.tensor(np.asarray(acts, np.float64), requires_grad=True)
    lp = torch.log_softmax(x, dim=2).transpose(0, 1)
    costs = torch.nn.functional.ctc_loss(lp, torch.tensor(np.asarray(labels, np.int64)), torch.tensor(np.asarray(il, np.int64)),
                                         torch.tensor(np.asarray(ll, np.int64)), blank=blank, reduction="none")
    w = torch.ones(len(il), dtype=torch.float64) if scale is None else torch.tensor(np.broadcast_to(np.asarray(scale, np.float64), (len(il),)).copy())
    fin = torch.isfinite(costs)
    (w * torch.where(fin, costs, torch.zeros_like(costs))).sum().backward()
    g = x.grad.numpy().copy()
    g[~fin.numpy()] = 0.0
    return costs.detach().numpy(), g


def collapse(path, blank=0):
    out, prev = [], blank
    for a in path:
        if a != blank and a != prev:
            out.append(a)
        prev = a
    return out


def brute_force_cost(x, y, blank=0):
    """-log of the summed probability of every one of the V^T frame labellings that collapses to y (T <= 6, V <= 4)."""
    T, V = x.shape
    assert T <= 6 and V <= 4
    p = np.exp(log_softmax(x))
    want, total = [int(v) for v in y], 0.0
    for path in itertools.product(range(V), repeat=T):
        if collapse(path, blank) == want:
            total += float(np.prod(p[np.arange(T), path]))
    return -np.log(total) if total > 0.0 else np.inf


def greedy(acts, il, blank=0):
    """The greedy rule: (tokens [B, T], frames [B, T], lengths [B]) int32, -1 beyond lengths."""
    B, T, _ = acts.shape
    tokens, frames, lengths = np.full((B, T), -1, np.int32), np.full((B, T), -1, np.int32), np.zeros(B, np.int32)
    best = np.argmax(acts, axis=2)  # the first of several maxima
    for b in range(B):
        n, prev = 0, blank
        for t in range(min(max(int(il[b]), 0), T)):
            a = int(best[b, t])
            if a != blank and a != prev:
                tokens[b, n], frames[b, n] = a, t
                n += 1
            prev = a
        lengths[b] = n
    return tokens, frames, lengths


# ---- input builders -----------------------------------------------------------------------------------------------------
def random_labels(rng, L, V, blank=0, repeat_prob=0.2):
    """L labels without the blank; a label repeats its predecessor with probability repeat_prob."""
    symbols = np.array([v for v in range(V) if v != blank], np.int32)
    y = symbols[rng.integers(0, symbols.size, size=L)]
    for k in range(1, L):
        if rng.random() < repeat_prob:
            y[k] = y[k - 1]
    return y.astype(np.int32)


def case(B, T, L, V, seed, sigma=1.0, blank=0, il=None, ll=None, repeat_prob=0.2):
    """(acts f32 [B, T, V], labels i32 [B, max(L, 1)], il, ll): full lengths unless given."""
    rng = np.random.default_rng(seed)
    acts = (sigma * rng.normal(size=(B, T, V))).astype(np.float32)
    labels = np.stack([random_labels(rng, max(L, 1), V, blank, repeat_prob) for _ in range(B)])
    il = np.full(B, T, np.int32) if il is None else np.asarray(il, np.int32)
    ll = np.full(B, L, np.int32) if ll is None else np.asarray(ll, np.int32)
    return acts, labels, il, ll


def trained_like_case(B, T, L, V, seed, blank=0, peak=12.0):
    """One dominant symbol per frame along a valid alignment of each utterance's labels (blanks between, each label held for a
    frame or two), small noise elsewhere."""
    rng = np.random.default_rng(seed)
    acts = rng.normal(size=(B, T, V)).astype(np.float32)
    labels = np.stack([random_labels(rng, L, V, blank) for _ in range(B)])
    for b in range(B):
        path = []
        for k in range(L):
            path += [blank, int(labels[b, k])]
        path.append(blank)
        while len(path) < T:  # stretch: repeat a random state's frame
            i = int(rng.integers(0, len(path)))
            path.insert(i, path[i])
        assert len(path) == T and collapse(path, blank) == [int(v) for v in labels[b]]
        acts[b, np.arange(T), path] += peak
    return acts, labels, np.full(B, T, np.int32), np.full(B, L, np.int32)


# the scripted greedy scenarios: (name, per-utterance frame scripts, blank, V).  A frame is the set of symbols that tie for the
# maximum (the lowest index wins).
GREEDY_SCRIPTS = [
    ("ties", [[(1, 2), (0, 3), (2, 3), (3,), (0, 1, 2, 3)]], 0, 4),
    ("repeats", [[(1,), (1,), (0,), (1,), (2,), (2,), (1,), (0,), (0,), (3,)]], 0, 4),
    ("all_blank", [[(2,), (2,), (2,), (2,)]], 2, 4),
    ("blank_last", [[(1,), (3,), (3,), (0,), (3,), (1,)]], 3, 4),
    ("ragged", [[(1,), (2,), (2,), (3,), (0,), (1,), (1,)], [(2,), (0,)], [(0,), (0,), (3,)], []], 0, 5),
]


def scripted_logits(script, V, T=None):
    """acts [B, T, V] with the scripted symbols at exactly the same maximal value, il [B]."""
    B = len(script)
    T = T or max(1, max(len(s) for s in script))
    rng = np.random.default_rng(len(script) * 131 + V)
    acts = rng.normal(size=(B, T, V)).astype(np.float32).clip(-2.0, 2.0)
    il = np.array([len(s) for s in script], np.int32)
    for b, frames in enumerate(script):
        for t, tie in enumerate(frames):
            acts[b, t, list(tie)] = 5.0
    return acts, il


# ---- the tier constants of csrc/rnnt_ctc.h ------------------------------------------------------------------------------
def header_constants():
    """The sweep tiers and tile widths the kernels are built with, read from the layout header."""
    text = open(os.path.join(ROOT, "rnnt-speech-recognition_amd", "csrc", "rnnt_ctc.h")).read()
    out = {}
    for name in ("kCtcWaveThreads", "kCtcWideThreads", "kCtcRowVec", "kCtcGradTile", "kCtcGreedyChunk"):
        out[name] = int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))
    for name in ("kCtcWaveK", "kCtcWideK"):
        out[name] = [int(v) for v in re.search(r"constexpr int " + name + r"\[\] = \{([^}]*)\};", text).group(1).split(",")]
    return out


def tier_boundaries():
    """(positions at which the sweep changes its positions per thread within a wavefront, the wavefront-to-workgroup switch, the
    boundaries of the workgroup tiers): positions = L + 1."""
    c = header_constants()
    wave = [c["kCtcWaveThreads"] * k for k in c["kCtcWaveK"]]
    wide = [c["kCtcWideThreads"] * k for k in c["kCtcWideK"]]
    assert wave[-1] < wide[0] or wave[-1] == c["kCtcWideThreads"]
    return wave[:-1], wave[-1], wide[:-1]
