"""Contextual biasing (hotword boosting) for the beam search decoders: the context graph of include/rnnt_bias.h (rnntBiasGraph), built
on the host from token-id phrases and uploaded once per device.

Scoring model.  The phrases form a trie; the arc into node n carries the boost of the phrases that run through it (the largest,
where phrases with different boosts share a prefix).  With

    gain(n)    = the sum of the boosts on the path root -> n
    kept(n)    = gain of the deepest phrase-END node among n and its ancestors (0 if there is none)
    pending(n) = gain(n) - kept(n)

a hypothesis in state s that emits v moves to n = the longest suffix of path(s) + (v,) that is a trie node, and collects

    gain(n) - gain(s)      if n is the child of s (the match goes on), else
    gain(n) - pending(s)   (the match breaks off: what was collected beyond the last completed phrase is taken back, and the
                            new, shorter match is paid for)

so at any time a hypothesis holds (what its completed phrases banked) + gain(state).  The blank moves nothing.  At the end of a
decode a hypothesis left in state q holds pending(q) it has not earned: its final score is score + fail_bias[q]
(`ContextGraph.finalize`).

One limitation, kept for the sake of a deterministic automaton with one state per hypothesis: a phrase that is completed only
as a proper SUFFIX of a longer live match -- (2, 3) inside 1, 2, 3 while (1, 2, 3, 9) is still being matched -- is not banked
at that moment; if the longer match then breaks off at a token that continues neither, its bonus goes with the rest.

Layout.  States are the trie nodes in breadth-first order, the root first.  Every state lists its own arcs and, merged in, the
arcs of the states on its fail (Aho-Corasick suffix) chain down to, but excluding, the root; the nearest state wins.  With that
the three-case transition of include/rnnt_bias.h is exact: listed arc; else the root's arc plus fail_bias[s]; else the root and
fail_bias[s] = -pending(s).
"""
from __future__ import annotations

import ctypes
import math
from collections import deque
from typing import Callable, Iterable, Optional, Sequence

import numpy as np

from . import _lib


class ContextGraph:
    """ContextGraph(phrases, boost=1.0, blank=0, vocab_size=V): phrases = sequences of token ids; boost a positive number, or
    one per phrase.  Boosts are rounded to f32 once, so that host and device add the same numbers.

    arc_offsets / arc_tokens / arc_next / arc_bias / fail_bias: the arrays of rnntBiasGraph (numpy, host).  delta(s, v) ->
    (next, beta): the transition, from those arrays.  struct(device) -> the ctypes rnntBiasGraph of device tensors (uploaded at
    the first call for a device, kept by the object)."""

    def __init__(self, phrases: Iterable[Sequence[int]], boost=1.0, blank: int = 0, vocab_size: Optional[int] = None):
        if vocab_size is None or int(vocab_size) < 1:
            raise ValueError("ContextGraph: vocab_size is required")
        V, blank = int(vocab_size), int(blank)
        if not 0 <= blank < V:
            raise ValueError(f"ContextGraph: blank {blank} outside the vocabulary of {V} symbols")
        phrases = [tuple(int(t) for t in p) for p in phrases]
        if isinstance(boost, (int, float, np.floating, np.integer)):
            boosts = [boost] * len(phrases)
        else:
            boosts = list(boost)
            if len(boosts) != len(phrases):
                raise ValueError(f"ContextGraph: {len(boosts)} boosts for {len(phrases)} phrases")
        for p, b in zip(phrases, boosts):
            if not p:
                raise ValueError("ContextGraph: empty phrase")
            if blank in p:
                raise ValueError(f"ContextGraph: phrase {p} holds the blank ({blank})")
            if min(p) < 0 or max(p) >= V:
                raise ValueError(f"ContextGraph: phrase {p} holds an id outside [0, {V})")
            if not (isinstance(b, (int, float, np.floating, np.integer)) and math.isfinite(b) and b > 0):
                raise ValueError(f"ContextGraph: boost {b!r} is not a finite positive number")
        boosts = [float(np.float32(b)) for b in boosts]
        self.blank, self.vocab_size, self.phrases, self.boosts = blank, V, phrases, boosts
        self._build()
        self._device = {}

    @classmethod
    def from_texts(cls, texts: Iterable[str], encode: Callable[[str], Sequence[int]], **kw) -> "ContextGraph":
        """encode(text) -> token ids (a subword encoder's encode)."""
        return cls([list(encode(t)) for t in texts], **kw)

    # ---- the trie, the suffix links and the merged arc lists
    def _build(self):
        child = [{}]       # node -> {token: node}
        arc_boost = [0.0]  # boost of the arc INTO the node
        is_end = [False]
        for p, b in zip(self.phrases, self.boosts):
            n = 0
            for t in p:
                if t not in child[n]:
                    child[n][t] = len(child)
                    child.append({})
                    arc_boost.append(0.0)
                    is_end.append(False)
                n = child[n][t]
                arc_boost[n] = max(arc_boost[n], b)
            is_end[n] = True
        N = len(child)
        # breadth-first numbering; gain / kept; fail links
        order, number = [0], {0: 0}
        gain, kept, fail = [0.0] * N, [0.0] * N, [0] * N
        queue = deque([0])
        while queue:
            s = queue.popleft()
            for t in sorted(child[s]):
                c = child[s][t]
                number[c] = len(order)
                order.append(c)
                gain[c] = gain[s] + arc_boost[c]
                kept[c] = gain[c] if is_end[c] else kept[s]
                f = fail[s]
                while s != 0 and t not in child[f] and f != 0:
                    f = fail[f]
                fail[c] = child[f][t] if s != 0 and t in child[f] else 0
                queue.append(c)
        offsets, tokens, nexts, biases = [0], [], [], []
        fail_bias = np.zeros(N, np.float32)
        for s in order:
            pending = gain[s] - kept[s]
            fail_bias[number[s]] = -pending
            arcs = {t: (c, gain[c] - gain[s]) for t, c in child[s].items()}
            f = fail[s] if s != 0 else 0
            while f != 0:
                for t, c in child[f].items():
                    if t not in arcs:
                        arcs[t] = (c, gain[c] - pending)
                f = fail[f]
            for t in sorted(arcs):
                tokens.append(t)
                nexts.append(number[arcs[t][0]])
                biases.append(arcs[t][1])
            offsets.append(len(tokens))
        self.num_states, self.num_arcs = N, len(tokens)
        self.arc_offsets = np.asarray(offsets, np.int32)
        self.arc_tokens = np.asarray(tokens, np.int32)
        self.arc_next = np.asarray(nexts, np.int32)
        self.arc_bias = np.asarray(biases, np.float32)
        self.fail_bias = fail_bias
        self._rows = {}

    # ---- the transition, from the arrays (what the kernels compute)
    def _find(self, s: int, v: int) -> int:
        lo, hi = int(self.arc_offsets[s]), int(self.arc_offsets[s + 1])
        a = lo + int(np.searchsorted(self.arc_tokens[lo:hi], v))
        return a if a < hi and self.arc_tokens[a] == v else -1

    def delta(self, s: int, v: int):
        """-> (next state, beta as np.float32)."""
        if v == self.blank:
            return s, np.float32(0.0)
        a = self._find(s, v)
        if a >= 0:
            return int(self.arc_next[a]), self.arc_bias[a]
        fb = self.fail_bias[s]
        if s != 0:
            a = self._find(0, v)
            if a >= 0:
                return int(self.arc_next[a]), np.float32(fb + self.arc_bias[a])
        return 0, fb

    def row(self, s: int):
        """-> (beta f32 [V], next i32 [V]) of state s for every symbol (cached)."""
        if s not in self._rows:
            beta = np.full(self.vocab_size, self.fail_bias[s], np.float32)
            nxt = np.zeros(self.vocab_size, np.int32)
            lo, hi = int(self.arc_offsets[0]), int(self.arc_offsets[1])
            beta[self.arc_tokens[lo:hi]] = (self.fail_bias[s] + self.arc_bias[lo:hi]) if s != 0 else self.arc_bias[lo:hi]
            nxt[self.arc_tokens[lo:hi]] = self.arc_next[lo:hi]
            if s != 0:
                lo, hi = int(self.arc_offsets[s]), int(self.arc_offsets[s + 1])
                beta[self.arc_tokens[lo:hi]] = self.arc_bias[lo:hi]
                nxt[self.arc_tokens[lo:hi]] = self.arc_next[lo:hi]
            beta[self.blank], nxt[self.blank] = 0.0, s
            self._rows[s] = (beta, nxt)
        return self._rows[s]

    def walk(self, tokens: Sequence[int], state: int = 0):
        """The state after `tokens` and the bias collected on the way (float64)."""
        total = 0.0
        for v in tokens:
            state, b = self.delta(state, int(v))
            total += float(b)
        return state, total

    def finalize(self, scores, states):
        """score + fail_bias[state]: what a hypothesis keeps when the decode ends in `state` (tensors or arrays, same shape)."""
        import torch

        if isinstance(scores, torch.Tensor):
            fb = torch.as_tensor(self.fail_bias, device=scores.device)
            return scores + fb[states.to(device=scores.device, dtype=torch.long)].to(scores.dtype)
        return np.asarray(scores) + self.fail_bias[np.asarray(states)]

    # ---- the device side
    def struct(self, device) -> "_lib.rnntBiasGraph":
        import torch

        device = torch.device(device)
        if device not in self._device:
            up = lambda x: torch.from_numpy(np.ascontiguousarray(x) if x.size else np.zeros(1, x.dtype)).to(device)  # noqa: E731
            t = [up(self.arc_offsets), up(self.arc_tokens), up(self.arc_next), up(self.arc_bias), up(self.fail_bias)]
            g = _lib.rnntBiasGraph(self.num_states, self.num_arcs, *[x.data_ptr() for x in t])
            self._device[device] = (g, t)  # (the tensors live as long as the struct)
        return self._device[device][0]

    def byref(self, device):
        return ctypes.byref(self.struct(device))
