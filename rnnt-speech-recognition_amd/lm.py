"""N-gram language-model shallow fusion for the beam search decoders: the automaton of include/rnnt_lm.h (rnntLmGraph), built on
the host from a back-off n-gram LM (an ARPA file, in-memory tables, or counts estimated from token-id sequences) and uploaded once
per device.

Scoring model.  A back-off LM lists n-grams h + (w,) with a log-probability, and histories h with a back-off weight:

    log P(w | h) = logp(h + (w,))                       if the n-gram is listed, else
                   bow(h) + log P(w | h[1:])            (bow(h) = 0 where h is not listed), down to the empty history, where
    log P(w | ()) = logp((w,)) if listed, else the unknown-token score.

A hypothesis that emits v collects scale * log P(v | its tokens so far, after <s>) + token_bonus; the blank moves nothing.  The
per-token bonus is folded into the arc scores and the unknown-token score, which is exact because every non-blank transition
ends in exactly one arc or in the unknown-token case.  At the end of a decode a hypothesis in state q is owed the
end-of-sentence score final_score[q] = scale * log P(</s> | history) (`NgramLM.finalize`); </s> is never an arc.

Layout.  A state is a history: every history that occurs as the context of a listed n-gram or carries a non-zero back-off
weight, plus the <s> history (state 0: where every hypothesis starts) and the empty history E (state 1).  The other states
follow by length, then lexicographically.  Histories that are no state have nothing to say (no listed continuation, no back-off
weight), so the automaton may skip them: arc_next of (h, v) is the longest suffix of h + (v,) that is a state, backoff_next of h
the longest PROPER suffix of h that is a state.  An LM without <s> n-grams leaves state 0 without arcs and with a back-off of
score 0 to E.  The longest chain has order - 1 hops, so the 8 hops of include/rnnt_lm.h take an LM of order 9 at most.

All additions of stored scores are f32 additions in the order include/rnnt_lm.h defines, here as in the kernels.
"""
from __future__ import annotations

import ctypes
import math
import os
from collections import defaultdict
from typing import Iterable, Mapping, Sequence

import numpy as np

from . import _lib

BOS, EOS, UNK = "<s>", "</s>", "<unk>"
MAX_HOPS = 8  # RNNT_LM_MAX_HOPS
_LN10 = math.log(10.0)


def _hist_key(h):
    return (len(h), tuple(-1 if t == BOS else t for t in h))


class NgramLM:
    """Built by from_arpa / from_ngrams / estimate.

    arc_offsets / arc_tokens / arc_next / arc_score / backoff_next / backoff_score, empty_state, unk_score: the fields of
    rnntLmGraph (numpy, host).  final_score f32 [S]: the scaled </s> score per state (zeros without </s> or with use_eos=False).
    histories: per state its history (a tuple of ids, "<s>" first where it applies); depth: its length.
    delta(s, v) -> (next, beta): the transition, from those arrays.  struct(device) -> the ctypes rnntLmGraph of device tensors
    (uploaded at the first call for a device, kept by the object)."""

    def __init__(self, ngrams: Mapping, blank: int, vocab_size: int, mult: float, token_bonus: float, unk: float, use_eos: bool):
        V, blank = int(vocab_size), int(blank)
        if V < 1:
            raise ValueError("NgramLM: vocab_size is required")
        if not 0 <= blank < V:
            raise ValueError(f"NgramLM: blank {blank} outside the vocabulary of {V} symbols")
        for name, x in (("scale", mult), ("token_bonus", token_bonus), ("the unknown-token score", unk)):
            if not math.isfinite(x):
                raise ValueError(f"NgramLM: {name} is not finite")
        self.blank, self.vocab_size = blank, V
        self._build(ngrams, float(mult), float(token_bonus), float(unk), bool(use_eos))
        self._device = {}
        self._rows = {}

    # ---- constructors
    @classmethod
    def from_ngrams(cls, ngrams: Mapping, blank: int, vocab_size: int, scale: float = 1.0, token_bonus: float = 0.0,
                    unk: float = -10.0, use_eos: bool = True, log10: bool = True) -> "NgramLM":
        """ngrams: {n-gram: (logp, bow)} or {n-gram: logp} (bow 0); an n-gram is a tuple of token ids with lm.BOS ("<s>") allowed
        first and lm.EOS ("</s>") last.  logp, bow and unk (a non-blank token the unigrams do not list) are log10 values as in an
        ARPA file, or natural logarithms with log10=False.  The logp of the unigram ("<s>",) is not used, its bow is."""
        return cls(ngrams, blank, vocab_size, scale * (_LN10 if log10 else 1.0), token_bonus, unk, use_eos)

    @classmethod
    def from_arpa(cls, text_or_path, token_to_id, blank: int, vocab_size: int, scale: float = 1.0, token_bonus: float = 0.0,
                  unk_log10: float = -10.0, use_eos: bool = True) -> "NgramLM":
        """A standard ARPA file (its text, or a path): log10 probabilities, optional back-off weights.  token_to_id: a mapping
        (or a callable) from the file's words to token ids; <s> and </s> are the sentence marks.  A unigram <unk> sets the
        unknown-token score (else unk_log10); n-grams of higher order that hold <unk> are dropped.  Any other word token_to_id
        does not know is an error."""
        text = text_or_path
        if "\\data\\" not in str(text_or_path):
            with open(os.fspath(text_or_path), "r", encoding="utf-8") as f:
                text = f.read()
        lookup = token_to_id if callable(token_to_id) else token_to_id.get
        ngrams, order, unk = {}, 0, float(unk_log10)
        for ln, line in enumerate(text.splitlines(), 1):
            line = line.strip()
            if not line or line == "\\data\\" or line.startswith("ngram "):
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                order = int(line[1:-len("-grams:")])
                continue
            parts = line.split()
            if order < 1 or len(parts) not in (order + 1, order + 2):
                raise ValueError(f"NgramLM.from_arpa: line {ln}: expected a log-probability, {order} words and an optional back-off weight")
            try:
                lp = float(parts[0])
                bow = float(parts[order + 1]) if len(parts) == order + 2 else 0.0
            except ValueError:
                raise ValueError(f"NgramLM.from_arpa: line {ln}: not a number") from None
            words = parts[1: order + 1]
            if UNK in words:
                if order == 1:
                    unk = lp
                continue
            gram = []
            for w in words:
                if w in (BOS, EOS):
                    gram.append(w)
                    continue
                t = lookup(w)
                if t is None:
                    raise ValueError(f"NgramLM.from_arpa: line {ln}: no token id for {w!r}")
                gram.append(int(t))
            ngrams[tuple(gram)] = (lp, bow)
        return cls(ngrams, blank, vocab_size, scale * _LN10, token_bonus, unk, use_eos)

    @classmethod
    def estimate(cls, sequences: Iterable[Sequence[int]], order: int, blank: int, vocab_size: int, discount: float = 0.75,
                 **scores) -> "NgramLM":
        """An LM of `order` from token-id sequences, each between <s> and </s>, by interpolated absolute discounting:

            P(w | h) = max(c(h w) - D, 0) / c(h) + D n(h) / c(h) * P(w | h[1:])     (n(h): the distinct words seen after h)
            P(w)     = max(c(w) - D, 0) / c + D n / c * 1 / V                       (uniform over the V - 1 tokens and </s>)

        in back-off form: every seen n-gram is listed with its full interpolated probability and h with bow(h) = D n(h) / c(h).
        Every non-blank token is a unigram, so nothing is unknown.  **scores: scale, token_bonus, use_eos as in from_ngrams."""
        V, blank, order, D = int(vocab_size), int(blank), int(order), float(discount)
        if not 1 <= order <= MAX_HOPS + 1:
            raise ValueError(f"NgramLM.estimate: order {order} outside 1 ... {MAX_HOPS + 1}")
        if not 0.0 < D < 1.0:
            raise ValueError("NgramLM.estimate: discount must lie in (0, 1)")
        counts = defaultdict(lambda: defaultdict(int))  # history -> word -> count
        for seq in sequences:
            seq = [int(t) for t in seq]
            if any(t == blank or not 0 <= t < V for t in seq):
                raise ValueError(f"NgramLM.estimate: sequence {seq} holds the blank or an id outside [0, {V})")
            padded = [BOS] + seq + [EOS]
            for i in range(1, len(padded)):
                for n in range(order):
                    if i - n < 0:
                        break
                    counts[tuple(padded[i - n: i])][padded[i]] += 1
        words = [v for v in range(V) if v != blank] + [EOS]
        prob = {}  # history -> {word: P(w | h)} for the listed words

        def p_of(h, w):  # the interpolated P(w | h) of any history
            while h and h not in prob:
                h = h[1:]
            return prob[h][w] if w in prob[h] else bow[h] * p_of(h[1:], w)

        bow = {}
        uni = counts.get((), {})
        c = sum(uni.values())
        lam = D * len(uni) / c if c else 1.0
        prob[()] = {w: (max(uni.get(w, 0) - D, 0.0) / c if c else 0.0) + lam / len(words) for w in words}
        for h in sorted((h for h in counts if h), key=_hist_key):
            c = sum(counts[h].values())
            bow[h] = D * len(counts[h]) / c
            prob[h] = {w: (k - D) / c + bow[h] * p_of(h[1:], w) for w, k in counts[h].items()}
        ngrams = {}
        for h, row in prob.items():
            for w, p in row.items():
                ngrams[h + (w,)] = (math.log(p), 0.0)
        for h, b in bow.items():
            if len(h) < order:
                lp = ngrams.get(h, (0.0, 0.0))[0]  # (("<s>",): listed for its back-off weight alone)
                ngrams[h] = (lp, math.log(b))
        return cls.from_ngrams(ngrams, blank, V, log10=False, **scores)

    # ---- the automaton
    def _build(self, ngrams, mult, bonus, unk, use_eos):
        V, blank = self.vocab_size, self.blank
        table = {}
        for g, val in ngrams.items():
            g = tuple(g)
            lp, bw = (val if isinstance(val, (tuple, list)) else (val, 0.0))
            if not g:
                raise ValueError("NgramLM: empty n-gram")
            if len(g) > MAX_HOPS + 1:
                raise ValueError(f"NgramLM: n-gram {g} of order {len(g)}: the back-off walk takes {MAX_HOPS} hops, order {MAX_HOPS + 1} at most")
            for i, t in enumerate(g):
                if t == BOS:
                    if i != 0:
                        raise ValueError(f"NgramLM: n-gram {g}: <s> anywhere but first")
                elif t == EOS:
                    if i != len(g) - 1:
                        raise ValueError(f"NgramLM: n-gram {g}: </s> anywhere but last")
                elif not isinstance(t, (int, np.integer)) or isinstance(t, bool):
                    raise ValueError(f"NgramLM: n-gram {g}: {t!r} is no token id")
                elif t == blank:
                    raise ValueError(f"NgramLM: n-gram {g} holds the blank ({blank})")
                elif not 0 <= t < V:
                    raise ValueError(f"NgramLM: n-gram {g} holds an id outside [0, {V})")
            lp, bw = float(lp), float(bw)
            if not math.isfinite(bw) or (g != (BOS,) and not math.isfinite(lp)):
                raise ValueError(f"NgramLM: n-gram {g}: a score that is not finite")
            table[tuple(t if t in (BOS, EOS) else int(t) for t in g)] = (lp, bw)
        for g in table:
            if len(g) > 1 and g[:-1] not in table:
                raise ValueError(f"NgramLM: n-gram {g} without its prefix {g[:-1]}")
        self.order = max((len(g) for g in table), default=1)
        f32 = np.float32
        states = {g[:-1] for g in table if len(g) > 1}
        states |= {g for g, (_, bw) in table.items() if bw != 0.0 and g[-1] != EOS and len(g) <= MAX_HOPS}
        states -= {(BOS,), ()}
        hist = [(BOS,), ()] + sorted(states, key=_hist_key)
        number = {h: i for i, h in enumerate(hist)}
        S = len(hist)

        def longest(seq, proper=False):
            for k in range(1 if proper else 0, len(seq) + 1):
                if seq[k:] in number:
                    return number[seq[k:]]
            raise AssertionError

        by_hist = defaultdict(list)
        for g, (lp, _) in table.items():
            if g[-1] not in (BOS, EOS):
                by_hist[g[:-1]].append((g[-1], lp))
        offsets, tokens, nexts, scs = [0], [], [], []
        bn, bs = np.zeros(S, np.int32), np.zeros(S, f32)
        for s, h in enumerate(hist):
            for v, lp in sorted(by_hist.get(h, ())):
                tokens.append(v)
                nexts.append(longest(h + (v,)))
                scs.append(f32(mult * lp + bonus))
            offsets.append(len(tokens))
            bn[s] = longest(h, proper=True) if h else s
            bs[s] = f32(mult * table[h][1]) if h in table else f32(0.0)
        self.histories, self.depth = hist, np.asarray([len(h) for h in hist], np.int32)
        self.num_states, self.num_arcs, self.empty_state = S, len(tokens), 1
        self.unk_score = f32(mult * unk + bonus)
        self.arc_offsets = np.asarray(offsets, np.int32)
        self.arc_tokens = np.asarray(tokens, np.int32)
        self.arc_next = np.asarray(nexts, np.int32)
        self.arc_score = np.asarray(scs, f32)
        self.backoff_next, self.backoff_score = bn, bs
        for a in (self.arc_score, self.backoff_score, np.asarray([self.unk_score])):
            if not np.isfinite(a).all():
                raise ValueError("NgramLM: a scaled score is not finite in f32")
        # </s>: per state by the back-off walk (no token bonus: it is no token of the hypothesis)
        self.final_score = np.zeros(S, f32)
        if use_eos and any(g[-1] == EOS for g in table):
            for s, h in enumerate(hist):
                acc, hop, cur = f32(0.0), 0, s
                while True:
                    g = hist[cur] + (EOS,)
                    if g in table or cur == self.empty_state:
                        last = f32(mult * table[g][0]) if g in table else f32(mult * unk)
                        self.final_score[s] = last if hop == 0 else f32(acc + last)
                        break
                    acc = bs[cur] if hop == 0 else f32(acc + bs[cur])
                    cur, hop = int(bn[cur]), hop + 1
        self._rows = {}

    # ---- the transition, from the arrays (what the kernels compute)
    def _find(self, s: int, v: int) -> int:
        lo, hi = int(self.arc_offsets[s]), int(self.arc_offsets[s + 1])
        a = lo + int(np.searchsorted(self.arc_tokens[lo:hi], v))
        return a if a < hi and self.arc_tokens[a] == v else -1

    def delta(self, s: int, v: int):
        """-> (next state, beta as np.float32): include/rnnt_lm.h, its order of f32 additions."""
        f32 = np.float32
        if v == self.blank:
            return s, f32(0.0)
        cur, hop, acc, E = s, 0, f32(0.0), self.empty_state
        while True:
            a = self._find(cur, v)
            if a >= 0:
                return int(self.arc_next[a]), self.arc_score[a] if hop == 0 else f32(acc + self.arc_score[a])
            if cur == E:
                return E, self.unk_score if hop == 0 else f32(acc + self.unk_score)
            acc = self.backoff_score[cur] if hop == 0 else f32(acc + self.backoff_score[cur])
            cur, hop = int(self.backoff_next[cur]), hop + 1
            if hop == MAX_HOPS:
                cur = E

    def row(self, s: int):
        """-> (beta f32 [V], next i32 [V]) of state s for every symbol (cached): the chain's levels, the farthest first."""
        if s not in self._rows:
            f32, E = np.float32, self.empty_state
            chain, cur, hop, acc = [(s, f32(0.0))], s, 0, f32(0.0)
            while cur != E:
                acc = self.backoff_score[cur] if hop == 0 else f32(acc + self.backoff_score[cur])
                cur, hop = int(self.backoff_next[cur]), hop + 1
                if hop == MAX_HOPS:
                    cur = E
                chain.append((cur, acc))
            d = len(chain) - 1
            beta = np.full(self.vocab_size, self.unk_score if d == 0 else f32(chain[d][1] + self.unk_score), f32)
            nxt = np.full(self.vocab_size, E, np.int32)
            for j in range(d, -1, -1):
                c, a = chain[j]
                lo, hi = int(self.arc_offsets[c]), int(self.arc_offsets[c + 1])
                beta[self.arc_tokens[lo:hi]] = self.arc_score[lo:hi] if j == 0 else (a + self.arc_score[lo:hi]).astype(f32)
                nxt[self.arc_tokens[lo:hi]] = self.arc_next[lo:hi]
            beta[self.blank], nxt[self.blank] = 0.0, s
            self._rows[s] = (beta, nxt)
        return self._rows[s]

    def walk(self, tokens: Sequence[int], state: int = 0):
        """The state after `tokens` and the LM score collected on the way (float64), without the </s> score."""
        total = 0.0
        for v in tokens:
            state, b = self.delta(state, int(v))
            total += float(b)
        return state, total

    def score(self, tokens: Sequence[int]) -> float:
        """The scaled score of a whole sentence: walk(tokens) and the </s> score of where it ends."""
        state, total = self.walk(tokens)
        return total + float(self.final_score[state])

    def finalize(self, scores, states):
        """score + final_score[state]: what a hypothesis holds when the decode ends in `state` (tensors or arrays, same shape)."""
        import torch

        if isinstance(scores, torch.Tensor):
            fs = torch.as_tensor(self.final_score, device=scores.device)
            return scores + fs[states.to(device=scores.device, dtype=torch.long)].to(scores.dtype)
        return np.asarray(scores) + self.final_score[np.asarray(states)]

    # ---- the device side
    def struct(self, device) -> "_lib.rnntLmGraph":
        import torch

        device = torch.device(device)
        if device not in self._device:
            up = lambda x: torch.from_numpy(np.ascontiguousarray(x) if x.size else np.zeros(1, x.dtype)).to(device)  # noqa: E731
            t = [up(self.arc_offsets), up(self.arc_tokens), up(self.arc_next), up(self.arc_score), up(self.backoff_next),
                 up(self.backoff_score)]
            g = _lib.rnntLmGraph(self.num_states, self.num_arcs, self.empty_state, float(self.unk_score), *[x.data_ptr() for x in t])
            self._device[device] = (g, t)  # (the tensors live as long as the struct)
        return self._device[device][0]

    def byref(self, device):
        return ctypes.byref(self.struct(device))
