"""Batched TDT beam search: a float64 restatement of the rule of include/rnnt_tdt_beam.h, scripted scenarios and the driver that
plays the caller (a helper module, not a conftest).

TDTBeamRestatement is written from the header text alone and shares nothing with tdt.TDTBeamJoint.  It works on the logits a
`logits_fn(b, t, tokens)` returns: [V + D] numbers, V token logits then D duration logits -- on the GPU the f32 logits of
compute_rnnt_joint_logits for that hypothesis alone with alphabet_size = V + D, on the CPU the script's own float64 table.  It
BRUTE-FORCES all V D candidates of every active hypothesis: neither the token top-K nor the pair top-K shortcut of the library and
of the torch route exists here, so the shortcuts are what gets tested.

A scenario is a tests/tdt_decode_cases.Case (W2 = c I over V + D columns, enc_proj = 0, pred_row(b, t, tokens)) plus a beam width.

Comparison rules (run_tdt_beam): ids, lengths, cursors, parents, emitted, frames and durations exactly, at EVERY step, nothing
skipped.  Scores within decode_scripts.score_bar(2 n, max |lse|, s) after n frames: each decision has two logsumexps.  A scenario
must keep any two adjacent deciding candidates, and any two neighbours of a new beam, either exactly tied (where it declares ties)
or more than twice that bar apart; the restatement asserts that on itself alone.

The key's levels: an exact tie is decided by the hypothesis i, then stay before tokens, then v, then j.  A hypothesis is either
active or waiting, so it never offers a stay AND a token: a stay that ties with a token belongs to another hypothesis and i decides.
The restatement sorts on the full key all the same; the scenarios force ties at the levels i, v and j, stays tied with stays
included.
"""
import math
from dataclasses import dataclass, field

import numpy as np

from tests import decode_scripts as ds
from tests import tdt_decode_cases as tc


def score_bar(n, max_lse, s):
    return ds.score_bar(2 * n, max_lse, s)


def _logaddexp(a, b):
    hi, lo = max(a, b), min(a, b)
    return hi + math.log1p(math.exp(lo - hi))


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
@dataclass
class Events:
    merges: int = 0             # taken candidates merged away
    stay_merges: int = 0        # ... in a group that holds a stay and an expansion
    d0_d1_merges: int = 0       # ... (i, v, 0) + (i, v, 1) with durations [0, 1, ...]
    kept_apart: int = 0         # pairs of a new beam with equal sequences and different cursors
    aligned_later: int = 0      # merges of members that arrive from different parents
    ties: int = 0
    tie_levels: set = field(default_factory=set)  # the level of the key that decided an exact tie: "i", "v", "j"
    carried: list = field(default_factory=list)   # (utterance, frame) where nothing could be taken
    dropped: int = 0            # active hypotheses without a finite candidate in a frame where something was taken
    idle_frames: int = 0        # (utterance, frame) pairs with t < T_b and no active hypothesis
    idle_full: int = 0          # ... with `beam` hypotheses waiting
    full_frames: int = 0
    past_end: int = 0           # new hypotheses whose cursor passed T_b
    active_rows: int = 0        # joint rows evaluated
    frames: int = 0             # (utterance, frame) pairs with t < T_b
    durations_used: set = field(default_factory=set)
    min_gap: float = math.inf
    max_lse: float = 0.0
    worst_gap_ratio: float = math.inf


class TDTBeamRestatement:
    """beams[b]: [(tokens, cursor, score, frames, durations)], best first."""

    def __init__(self, logits_fn, B, K, V, durations, frame_lengths, maxT, blank, ties_allowed=False):
        assert 0 <= blank < V and K >= 1
        self.fn, self.B, self.K, self.V, self.dur, self.blank = logits_fn, B, K, V, list(durations), blank
        self.ties_allowed = ties_allowed
        self.Tb = [min(max(int(f), 0), maxT) for f in frame_lengths]
        self.beams = [[((), 0, 0.0, (), ())] for _ in range(B)]
        self.t = 0
        self.ev = Events()

    def active(self, b, k):
        return self.t < self.Tb[b] and k < len(self.beams[b]) and self.beams[b][k][1] == self.t

    def _gap(self, hi, lo, n, what, level=None):
        gap = hi - lo
        if gap == 0.0:
            assert self.ties_allowed, f"scenario precondition: unintended exact tie ({what})"
            self.ev.ties += 1
            if level:
                self.ev.tie_levels.add(level)
            return
        bar = score_bar(n, self.ev.max_lse, max(abs(hi), abs(lo)))
        self.ev.min_gap = min(self.ev.min_gap, gap)
        self.ev.worst_gap_ratio = min(self.ev.worst_gap_ratio, gap / (2 * bar))
        assert gap > 2 * bar, f"scenario precondition: candidates {gap:.3e} apart, bar {bar:.3e} ({what})"

    def step(self):
        """One frame of every utterance -> (parents, emitted) as the library must write them."""
        K, V, t, ev = self.K, self.V, self.t, self.ev
        D = len(self.dur)
        parents, emitted = list(range(self.B * K)), [-1] * (self.B * K)
        for b in range(self.B):
            if t >= self.Tb[b]:
                continue
            beam = self.beams[b]
            assert all(h[1] >= t for h in beam), "invariant: every cursor >= t"
            ev.frames += 1
            ev.full_frames += len(beam) == K
            cands = []  # (score, i, stay first: 0 / 1, v, j)
            nact, finite = 0, {}
            for i, (y, c, s, fr, du) in enumerate(beam):
                if c != t:
                    cands.append((s, i, 0, -1, -1))
                    continue
                nact += 1
                lg = np.asarray(self.fn(b, t, y), np.float64)
                assert lg.shape == (V + D,)
                lse_t, lse_d = tc._logsumexp(lg[:V]), tc._logsumexp(lg[V:])
                for x in (lse_t, lse_d):
                    if math.isfinite(x):
                        ev.max_lse = max(ev.max_lse, abs(x))
                # all V D scores, the additions in the header's order; the whole table is sorted under (score desc, v, j) and only
                # its first K + 1 entries go on: no later one can be among the first K + 1 of the utterance
                with np.errstate(invalid="ignore"):
                    sc = s + ((lg[:V, None] - lse_t) + (lg[None, V:] - lse_d))
                ok = np.flatnonzero((sc == sc) & (sc > -math.inf))
                finite[i] = len(ok)
                vv, jj = ok // D, ok % D
                flat = sc.reshape(-1)[ok]
                for n in np.lexsort((jj, vv, -flat))[: K + 1]:
                    cands.append((float(flat[n]), i, 1, int(vv[n]), int(jj[n])))
            ev.active_rows += nact
            if nact == 0:
                ev.idle_frames += 1
                ev.idle_full += len(beam) == K
            cands.sort(key=lambda x: (-x[0], x[1], x[2], x[3], x[4]))
            for r in range(min(K, len(cands) - 1)):  # the pairs that decide membership and order
                p, q = cands[r], cands[r + 1]
                level = "i" if p[1] != q[1] else ("v" if p[3] != q[3] else "j")
                self._gap(p[0], q[0], t + 1, f"utterance {b} frame {t} rank {r}", level)
            taken = cands[:K]
            if not taken:
                ev.carried.append((b, t))
                self.beams[b] = [(y, t + 1, s, fr, du) for y, c, s, fr, du in beam]
                continue
            ev.dropped += sum(1 for n in finite.values() if n == 0)
            new = []  # [tokens, cursor, score, frames, durations, parent, emitted, members], in rank order
            for sc, i, kind, v, j in taken:
                y, c, _, fr, du = beam[i]
                em = -1
                if kind == 1:
                    d = self.dur[j]
                    ev.durations_used.add(d)
                    if d == 0:
                        d = 1
                    c = t + d
                    if v != self.blank:
                        y, fr, du, em = y + (v,), fr + (t,), du + (d,), v
                for e in new:
                    if e[0] == y and e[1] == c:
                        e[2] = _logaddexp(e[2], sc)
                        e[7].append((i, kind, v, j))
                        ev.merges += 1
                        break
                else:
                    new.append([y, c, sc, fr, du, i, em, [(i, kind, v, j)]])
            for e in new:
                mem = e[7]
                if len(mem) > 1:
                    kinds = {m[1] for m in mem}
                    ev.stay_merges += kinds == {0, 1}
                    ev.aligned_later += len({m[0] for m in mem}) > 1
                    for m in mem[1:]:
                        first = mem[0]
                        ev.d0_d1_merges += (m[0], m[2]) == (first[0], first[2]) and m[1] == first[1] == 1 and \
                            {self.dur[m[3]], self.dur[first[3]]} == {0, 1}
            order = sorted(range(len(new)), key=lambda n: -new[n][2])  # (stable)
            new = [new[n] for n in order]
            for n in range(len(new) - 1):
                self._gap(new[n][2], new[n + 1][2], t + 1, f"utterance {b} frame {t} new beam {n}")
            for x in range(len(new)):
                ev.past_end += new[x][1] > self.Tb[b] and new[x][7][0][1] == 1
                for z in range(x + 1, len(new)):
                    ev.kept_apart += new[x][0] == new[z][0] and new[x][1] != new[z][1]
            self.beams[b] = [tuple(e[:5]) for e in new]
            for k, e in enumerate(new):
                parents[b * K + k], emitted[b * K + k] = b * K + e[5], e[6]
        self.t += 1
        return parents, emitted


# ---------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------
def run_tdt_beam(engine, sc, logits_fn, check=True, every_step=True):
    """Play the caller of compute_rnnt_tdt_beam_*: `engine` has begin(), step(rows [B K, J]) -> (parents, emitted) and results()
    -> (hyps [B, K, maxT], lengths, scores, cursors, frames, durations), all numpy.  Rows that are not active get NaN pred_proj:
    they must read nothing.  With check, every step's outputs AND results are held against the restatement.
    -> (trace, restatement, worst score error, its bar)."""
    case, K = sc.case, sc.K
    B = case.B
    ref = TDTBeamRestatement(logits_fn, B, K, case.V, case.durations, case.frames, case.maxT, case.blank, case.ties_allowed)
    seqs = [()] * (B * K)
    trace = []
    worst, worst_bar = 0.0, 0.0
    engine.begin()

    def compare(n_steps):
        nonlocal worst, worst_bar
        hyps, lengths, scores, cursors, frames, durs = engine.results()
        trace.append(tuple(np.array(x).copy() for x in (hyps, lengths, scores, cursors, frames, durs)))
        if not check:
            return
        for b in range(B):
            beam = ref.beams[b]
            n = min(n_steps, ref.Tb[b])
            for k in range(K):
                at = (n_steps, b, k)
                if k >= len(beam):
                    assert lengths[b, k] == 0 and scores[b, k] == -math.inf and not hyps[b, k].any() and cursors[b, k] == -1, (at, "empty")
                    assert (frames[b, k] == -1).all() and (durs[b, k] == -1).all(), (at, "empty slot's times")
                    continue
                y, c, s, fr, du = beam[k]
                L = len(y)
                assert lengths[b, k] == L and hyps[b, k, :L].tolist() == list(y) and not hyps[b, k, L:].any(), (at, "ids")
                assert cursors[b, k] == c, (at, "cursor", int(cursors[b, k]), c)
                assert frames[b, k, :L].tolist() == list(fr) and (frames[b, k, L:] == -1).all(), (at, "frames")
                assert durs[b, k, :L].tolist() == list(du) and (durs[b, k, L:] == -1).all(), (at, "durations")
                assert seqs[b * K + k] == y, (at, "the caller's sequence")
                err, bar = abs(float(scores[b, k]) - s), score_bar(max(n, 1), ref.ev.max_lse, s)
                assert err <= bar, (at, "score", float(scores[b, k]), s, err, bar)
                if err >= worst:
                    worst, worst_bar = err, bar

    for step in range(sc.steps):
        rows = np.full((B * K, case.J), np.nan, np.float32)
        for r in range(B * K):
            b, k = divmod(r, K)
            if ref.active(b, k):
                rows[r] = case.pred_row(b, step, seqs[r])
        parents, emitted = engine.step(rows)
        trace.append((np.array(parents).copy(), np.array(emitted).copy()))
        seqs = [seqs[p] + ((e,) if e >= 0 else ()) for p, e in zip(parents.tolist(), emitted.tolist())]
        want_p, want_e = ref.step()
        if check:
            assert parents.tolist() == want_p, (step, "parents", parents.tolist(), want_p)
            assert emitted.tolist() == want_e, (step, "emitted", emitted.tolist(), want_e)
        if every_step or step + 1 == sc.steps:
            compare(step + 1)
    if sc.steps == 0:
        compare(0)
    return trace, ref, worst, worst_bar


def dry_run(sc, logits_fn):
    """The restatement alone (its own beams are the caller's sequences) -> the restatement; raises where a precondition fails."""
    case = sc.case
    ref = TDTBeamRestatement(logits_fn, case.B, sc.K, case.V, case.durations, case.frames, case.maxT, case.blank, case.ties_allowed)
    for _ in range(sc.steps):
        ref.step()
    return ref


traces_equal = tc.traces_equal


# ---------------------------------------------------------------------------------------------
# scripts: (b, t, tokens) -> [V + D] float64
# ---------------------------------------------------------------------------------------------
def _u(n, *key):
    return np.random.default_rng([int(k) for k in key]).random(n)


def random_script(seed, V, D, blank, spread=3.0, ydep=0.5, dspread=2.0, nan=None):
    """Frame-dependent random logits in both heads, the same for every hypothesis of an utterance up to a shift of the token head by
    its last token and of the duration head by its length: hypotheses with a common history meet the same entries, so sequences
    re-join (merges) and jumps of different lengths re-align.  A likely blank.  nan(b, t, y) -> True: a NaN row there."""
    cache = {}

    def script(b, t, y):
        if nan is not None and nan(b, t, y):
            return np.full(V + D, np.nan)
        last = y[-1] if y else V
        key = (b, t, last, len(y) % 2)
        if key not in cache:
            L = np.empty(V + D)
            L[:V] = -spread * _u(V, seed, b, t) - ydep * _u(V, seed + 1, b, t, last)
            L[blank] *= 0.15
            L[V:] = -dspread * _u(D, seed + 2, b, t) - 0.3 * _u(D, seed + 3, b, t, len(y) % 2)
            cache[key] = L
        return cache[key]

    return script


def d0_d1_script(V, D, blank):
    """Durations [0, 1, ...]: at every frame one token p (the blank at every third frame) well ahead, and the durations 0 and 1 close
    together ahead of the rest: (i, p, 0) and (i, p, 1) both move one frame on and merge."""
    assert blank == 0

    def script(b, t, y):
        L = np.empty(V + D)
        L[:V] = -7.0 - 0.31 * np.arange(V) - 0.2 * _u(V, 11, b, t, len(y))
        L[blank if t % 3 == 2 else 1 + (t + b) % (V - 1)] = 0.0
        L[V:] = -8.0 - 0.37 * np.arange(D) - 0.2 * _u(D, 12, b, t, len(y))
        L[V], L[V + 1] = -0.23 * (1 + t % 2), -0.11 * (1 + (t + 1) % 2)
        return L

    return script


def wait_merge_script(V, D, blank, j_short, j_long):
    """The blank ahead at every frame, with the jumps durations[j_short] (= 1) and durations[j_long] both likely: (y, t + 1) and
    (y, t + long) are kept apart; the early hypothesis then walks up to the waiting one frame by frame, and the expansion that lands
    on its cursor merges with its stay.  A token 2.7 behind keeps a second sequence in a wider beam."""
    assert blank == 0

    def script(b, t, y):
        L = np.empty(V + D)
        L[:V] = -9.0 - 0.29 * np.arange(V) - 0.2 * _u(V, 13, b, t, len(y))
        L[blank] = 0.0
        L[1 + (len(y) + b) % (V - 1)] = -2.7 - 0.13 * (t % 3)
        L[V:] = -9.0 - 0.41 * np.arange(D) - 0.2 * _u(D, 14, b, t, len(y))
        L[V + j_short], L[V + j_long] = -0.17, -0.59 - 0.07 * (t % 2)
        return L

    return script


def key_tie_script(V, D, blank, p, q, ja, jb):
    """Every hypothesis of a frame gets the same row: tokens p < q tied at the top and durations ja < jb (both > 0, different
    jumps) tied at the top, so (p, ja), (p, jb), (q, ja), (q, jb) tie exactly: the key orders them by v, then j.  Next frame the
    hypotheses with the short jump are active with equal scores and equal rows (ties across i), the others wait with equal scores
    (stays tied: i decides)."""
    def script(b, t, y):
        L = np.empty(V + D)
        L[:V] = -6.0 - 0.07 * np.arange(V) - 0.05 * t
        L[V:] = -7.0 - 0.19 * np.arange(D)
        L[p] = L[q] = 0.0
        L[V + ja] = L[V + jb] = 0.0
        return L

    return script


def long_jump_script(V, D, blank, j_big):
    """The largest duration far ahead of the others at every frame: the whole beam jumps together, the frames between are idle (no
    hypothesis is active) with a full beam, and the last jump passes T_b.  Tokens: a fan of close candidates."""
    def script(b, t, y):
        L = np.empty(V + D)
        L[:V] = -0.35 * ((np.arange(V) + t + b + len(y)) % V) - 0.11 * _u(V, 7, b, t, len(y), y[-1] if y else V)
        L[V:] = -9.0 - 0.3 * np.arange(D)
        L[V + j_big] = 0.0
        return L

    return script


def collision_script(seq0, seq1, blank):
    """ds.collision_script on the token head (V = 7) and one duration (d = 1)."""
    base = ds.collision_script(7, seq0, seq1, blank)

    def script(b, t, y):
        return np.concatenate([base(b, t, y), [0.0]])

    return script


# ---------------------------------------------------------------------------------------------
# scenarios (shared by the CPU run on the torch route and the GPU runs through the C ABI and through Python)
# ---------------------------------------------------------------------------------------------
@dataclass
class Scenario:
    name: str
    case: object  # tests/tdt_decode_cases.Case
    K: int
    steps: int
    expect: dict = field(default_factory=dict)  # lower bounds on Events fields; "carried": the exact list; sets: subsets


def _scenario(name, dtype, V, durations, B, maxT, frames, blank, script, K, steps=None, ties_allowed=False, expect=None):
    case = tc.scripted_case(name, dtype, V, durations, B, maxT, frames, None, 1, blank, script, [maxT], ties_allowed=ties_allowed)
    return Scenario(name, case, K, maxT if steps is None else steps, expect or {})


D012, D5 = [0, 1, 2], [0, 1, 2, 3, 4]
RAGGED = [9, 0, 1, 12, 5]  # T_b = 0, T_b = 1, a length above maxT


def d0_d1_scenario(K, dtype=0):
    return _scenario(f"d0-d1-merge-K{K}-dt{dtype}", dtype, 8, D012, 5, 9, RAGGED, 0, d0_d1_script(8, 3, 0), K,
                     expect=dict(d0_d1_merges=6 if K > 1 else 0, merges=6 if K > 1 else 0))


def wait_merge_scenario(K, dtype=0):
    return _scenario(f"wait-merge-K{K}-dt{dtype}", dtype, 7, [1, 2, 4], 5, 9, RAGGED, 0, wait_merge_script(7, 3, 0, 0, 1), K,
                     expect=dict(stay_merges=2 if K > 1 else 0, kept_apart=2 if K > 1 else 0, aligned_later=2 if K > 1 else 0))


def key_tie_scenario(K, dtype=0):
    V, p, q = (100, 5, 40) if dtype else (9, 3, 6)
    return _scenario(f"key-ties-K{K}-dt{dtype}", dtype, V, D012, 3, 6, [6, 8, 1], 0, key_tie_script(V, 3, 0, p, q, 1, 2), K,
                     ties_allowed=True, expect=dict(ties=4, tie_levels={"i", "v", "j"} if K >= 4 else {"v"} if K > 1 else set()))


def long_jump_scenario(K, dtype=0):
    return _scenario(f"long-jumps-K{K}-dt{dtype}", dtype, 20, [0, 1, 4], 4, 10, [10, 7, 0, 1], 2, long_jump_script(20, 3, 2, 2), K,
                     expect=dict(idle_frames=6, idle_full=4, past_end=1))


def nan_scenario(K=4, dtype=0):
    """Utterance 1 is all NaN at frame 0 (its one hypothesis is active: nothing taken); with the single duration 1 every hypothesis
    is always active, so the NaN frame 4 of utterance 3 carries a full beam over.  Utterance 0: from frame 3 on the hypotheses of
    odd length are NaN, the others are not (dropped)."""
    nan = lambda b, t, y: (b, t) in ((1, 0), (3, 4)) or (b == 0 and t >= 3 and len(y) % 2 == 1)  # noqa: E731
    return _scenario(f"nan-rows-K{K}-dt{dtype}", dtype, 7, [1], 5, 8, [8, 8, 0, 8, 1], 0, random_script(NAN_SEED, 7, 1, 0, nan=nan), K,
                     expect=dict(carried=[(1, 0), (3, 4)], dropped=1))


def random_scenario(durations, K, dtype=0, seed=None, V=9, blank=0):
    """A ragged batch (tdt_decode_cases.duration_set_case's frame lengths) of random rows over one duration set."""
    seed = RANDOM_SEEDS.get((tuple(durations), K, dtype, blank), 100) if seed is None else seed
    frames = [24, 0, 1, 27, 5, 2, 24]
    return _scenario(f"random-{durations}-K{K}-dt{dtype}-blank{blank}", dtype, V, durations, 7, 24, frames, blank,
                     random_script(seed, V, len(durations), blank), K, steps=12, expect=dict(merges=1 if K > 1 else 0))


def collision_scenario():
    """-> scenario, and the two sequences of 256 + 1024 tokens it must end with (the Thue-Morse pair: equal length, equal rolling
    hash, equal cursor, different tokens: they must NOT merge)."""
    s0, s1 = ds.thue_morse(1024, 1, 3)
    T = 1288
    sc = _scenario("hash-collision", 0, 7, [1], 2, T, [T + 5, 20], 0, collision_script(s0, s1, 0), 2)
    return sc, (2,) * 256 + s0, (2,) * 256 + s1


NAN_SEED = 3
# picked on the restatement alone, on the scripts' own float64 logits (tests/test_tdt_beam.py asserts the gap condition with room)
# with room: the first seed from 100 on whose smallest gap is above 6 x (2 bar) and that merges.  (durations, K, joint_dtype, blank)
# 100 everywhere but here
RANDOM_SEEDS = {((0, 1, 2), 4, 0, 0): 104, ((0, 1, 2), 16, 0, 0): 110, ((0, 1, 2), 4, 1, 0): 101, ((0, 1, 2, 3, 4), 16, 1, 0): 111,
                ((0, 1, 2), 16, 1, 0): 110}


RANDOM_KEYS = [(tuple(d), K, 0) for d in tc.DURATION_SETS for K in ((4,) if d != [0, 1, 2, 3, 4] else (1, 2, 4, 16))] + \
    [((0, 1, 2, 3, 4), 4, 4), ((1, 2), 4, 8), ((0, 1, 2), 16, 0)]  # (durations, K, blank): blank first, middle, last


def scripted_scenarios(dtype):
    """Every scripted scenario but the hash collision (its own test: 1288 frames), for one joint_dtype."""
    out = []
    for K in (1, 2, 4, 16):
        out += [d0_d1_scenario(K, dtype), wait_merge_scenario(K, dtype), key_tie_scenario(K, dtype), long_jump_scenario(K, dtype)]
    out += [nan_scenario(4, dtype), nan_scenario(2, dtype)]
    # every duration set of tdt_decode_cases.duration_set_case with the blank first; the blank in the middle and last on two more
    out += [random_scenario(list(d), K, dtype, blank=blank) for d, K, blank in RANDOM_KEYS]
    return out


def check_expectations(sc, ev):
    for key, want in sc.expect.items():
        got = getattr(ev, key)
        if key == "carried":
            assert got == want, (sc.name, key, got, want)
        elif isinstance(want, set):
            assert want <= got, (sc.name, key, got, want)
        else:
            assert got >= want, (sc.name, key, got, want)


def describe(sc, ev, worst, bar):
    gap = "-" if ev.min_gap == math.inf else f"{ev.min_gap:.3g}"
    ratio = "-" if ev.worst_gap_ratio == math.inf else f"{ev.worst_gap_ratio:.3g}"
    return (f"[{sc.name}] merges={ev.merges} (stay+expansion {ev.stay_merges}, d0+d1 {ev.d0_d1_merges}, from two parents "
            f"{ev.aligned_later}) kept-apart={ev.kept_apart} ties={ev.ties} {sorted(ev.tie_levels)} carried={ev.carried} "
            f"dropped={ev.dropped} idle-frames={ev.idle_frames} (full beam {ev.idle_full}) past-end={ev.past_end} "
            f"active-rows={ev.active_rows}/{ev.frames} frames durations={sorted(ev.durations_used)} min-gap={gap} "
            f"gap/2bar={ratio} score-error={worst:.3e} bar={bar:.3e}")
