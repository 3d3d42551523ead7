"""The ordered band-position rule of include/rnnt_prune_ranges.h restated in plain loops, and the cases of its tests.

`ranges` is the definition as loops: per frame, for s0 = 0 ... hi, the window's S terms are added one by one, in increasing s,
into a float64 accumulator (a Python float is an IEEE binary64), and a candidate replaces the best so far only when w > best,
from (-inf, 0); steps 2 - 5 are loops as well.  Nothing in it is vectorised, so it shares no order of additions with torch."""
import numpy as np

NEG_INF = float("-inf")


def clamp_lengths(il, ll, T, U, S):
    """(T_b, L_b, hi) per utterance, as the rule clamps them."""
    Tb = [min(max(int(x), 1), T) for x in il]
    Lb = [min(max(int(x), 0), U - 1) for x in ll]
    return Tb, Lb, [max(0, L + 1 - S) for L in Lb]


def ranges(occ, il, ll, S):
    """s_begin [B, T] int32 of occupancies [B, T, U] (any float dtype: each term is widened to float64)."""
    occ = np.asarray(occ)
    B, T, U = occ.shape
    Tbs, Lbs, his = clamp_lengths(il, ll, T, U, S)
    out = np.empty((B, T), np.int32)
    for b in range(B):
        Tb, Lb, hi = Tbs[b], Lbs[b], his[b]
        sb = [0] * Tb
        for t in range(Tb):
            best, at = NEG_INF, 0
            if hi > 0:  # (hi = 0: the answer is 0 and nothing is read)
                row = [float(x) for x in occ[b, t, :Lb + 1]]  # nothing beyond L_b is read
                for s0 in range(hi + 1):
                    w = row[s0]
                    for k in range(1, S):
                        w = w + row[s0 + k]
                    if w > best:
                        best, at = w, s0
            sb[t] = at
        sb[0] = 0
        sb[Tb - 1] = hi
        for t in range(1, Tb):
            sb[t] = max(sb[t], sb[t - 1])
        for t in range(Tb - 2, 0, -1):
            sb[t] = max(sb[t], sb[t + 1] - (S - 1))
        out[b, :Tb] = sb
        out[b, Tb:] = hi
    return out


def check_invariants(sb, il, ll, S, U):
    """sb[0] = 0, sb[T_b - 1] = hi, non-decreasing, steps of at most S - 1, hi beyond T_b."""
    sb = np.asarray(sb)
    B, T = sb.shape
    Tbs, _, his = clamp_lengths(il, ll, T, U, S)
    for b in range(B):
        Tb, hi = Tbs[b], his[b]
        live = sb[b, :Tb].astype(np.int64)
        assert live[0] == (0 if Tb > 1 else hi) and live[-1] == hi, (b, live)
        d = np.diff(live)
        assert (d >= 0).all(), (b, live)
        # the first frame is pinned to 0 and is not part of step 4: the step out of it may be larger
        assert (d[1:] <= max(S - 1, 0)).all(), (b, live)
        assert (sb[b, Tb:] == hi).all(), (b, sb[b])


def ragged_lengths(B, T, U, S, rng):
    """Lengths with the rule's edges: a full utterance, T_b = 1 with L_b = 0, L_b + 1 < S, L_b + 1 = S, and random ones."""
    il = rng.integers(1, T + 1, size=B).astype(np.int32)
    ll = rng.integers(0, U, size=B).astype(np.int32)
    il[0], ll[0] = T, U - 1
    if B > 1:
        il[1], ll[1] = 1, 0
    if B > 2:
        ll[2] = min(max(S - 2, 0), U - 1)  # L_b + 1 < S (or as near as U allows): hi = 0
    if B > 3:
        ll[3] = min(S - 1, U - 1)          # L_b + 1 = S: hi = 0, the whole row is one window
    if B > 4:
        il[4] = T
    if B > 5:
        ll[5] = U - 1
    return il, ll


def random_case(B, T, U, S, seed):
    """Uniform float32 occupancies (ties are improbable) with ragged lengths."""
    rng = np.random.default_rng(seed)
    il, ll = ragged_lengths(B, T, U, S, rng)
    return rng.random((B, T, U), dtype=np.float32), il, ll


def exact_case(B, T, U, S, seed):
    """Multiples of 1/4 in [0, 1), plus all-zero and all-equal rows: every order of additions gives the same sum, and ties are
    everywhere."""
    rng = np.random.default_rng(seed)
    il, ll = ragged_lengths(B, T, U, S, rng)
    occ = (rng.integers(0, 4, size=(B, T, U)) / 4.0).astype(np.float32)
    for b in range(B):
        for t in range(T):
            kind = rng.integers(0, 4)
            if kind == 0:
                occ[b, t] = 0.0
            elif kind == 1:
                occ[b, t] = 0.25 * rng.integers(0, 4)
    return occ, il, ll


def peaked_case(B, T, U, S, seed):
    """Rows built by hand: 1.0 at a random column, flanked by values of 1e-17 ... 1e-20 on either side -- two windows that both
    hold the peak differ by less than an ulp of 1, and the order of additions decides which sum is larger."""
    rng = np.random.default_rng(seed)
    il, ll = ragged_lengths(B, T, U, S, rng)
    occ = (10.0 ** rng.uniform(-20.0, -17.0, size=(B, T, U))).astype(np.float32)
    for b in range(B):
        for t in range(T):
            occ[b, t, rng.integers(0, int(ll[b]) + 1)] = 1.0
    return occ, il, ll


def simple_inputs(B, T, U, V, seed):
    """3 N(0,1) inputs of the simple loss with ragged lengths: (am, lm, labels, il, ll) as numpy arrays."""
    rng = np.random.default_rng(seed)
    am = (3.0 * rng.normal(size=(B, T, V))).astype(np.float32)
    lm = (3.0 * rng.normal(size=(B, U, V))).astype(np.float32)
    labels = rng.integers(1, V, size=(B, max(U - 1, 1))).astype(np.int32)[:, :U - 1 if U > 1 else 1]
    il = rng.integers(max(T // 2, 1), T + 1, size=B).astype(np.int32)
    ll = rng.integers(U // 2, U, size=B).astype(np.int32)
    il[0], ll[0] = T, U - 1
    return am, lm, labels, il, ll
