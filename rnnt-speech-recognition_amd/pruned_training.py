"""The pruned training objective: the two-pass (k2-style) pruned transducer loss as a module that trains a Transducer.

    simple, pruned, s_begin = rnnt_loss_two_pass_fused(am, lm, enc_proj, pred_proj, W2, b2, ..., ordered_ranges=True)
    objective = simple_loss_scale * simple + pruned_loss_scale * pruned                      (per utterance)

The first pass is the simple (additive joiner) loss on two extra heads, am = am_head(enc) [B, T, V] and lm = lm_head(pred)
[B, U, V]; its occupancies give each frame's band of `s_range` symbols (prune_ranges with the ordered rule: the same occupancies
give the same band on every route); the second pass is the model's own joint on that band alone
(rnnt_joint_loss_pruned).  The reference's joint is Dense(tanh) on the broadcast sum (model.py:158-166), so JointLoss' parameters
serve the band unchanged: enc_proj = enc @ W1 + b1, pred_proj = pred @ W1, logits = tanh(enc_proj[t] + pred_proj[u]) @ W2 + b2.
The two projections and the two heads are torch matmuls under autograd; the three operators between them are the library's.

PrunedJointLoss owns the two heads and nothing else: the joint is an ARGUMENT of forward, its parameters are not registered a
second time, and state_dict() gains only `am_head.*` and `lm_head.*`."""
from __future__ import annotations

import torch
from torch import nn

from .loss import check_topology
from .pruned_joint import MAX_ALPHABET_SIZE, MAX_JOINT_SIZE, rnnt_loss_two_pass_fused
from .pruning import MAX_S_RANGE
from .simple import check_simple_scales


class PrunedJointLoss(nn.Module):
    """am_head, lm_head = nn.Linear(hidden, V) and the settings of the two-pass loss.  `simple_loss_scale` and `pruned_loss_scale`
    are plain attributes: a recipe may warm them up between steps.  After every forward, `last_simple_costs`, `last_pruned_costs`
    (detached, [B]) and `last_s_begin` ([B, T] int32) hold that call's parts, for logging and tests.

    A band that does not connect (0, 0) to the end costs +inf, with zero gradients from the second pass (rnnt_loss_pruned's contract):
    the rule of prune_ranges does not limit the step out of frame 0, so an untrained first pass whose occupancy at frame 1 peaks
    beyond column s_range - 1 gives such a band (profiles/prune_ranges_notes.md) -- watch `last_pruned_costs` during warm-up.

    ValueError at construction when the joint size or the vocabulary is outside what rnnt_joint_loss_pruned takes: joint_size a
    multiple of 64 up to 640, 2 <= vocab_size <= 8192."""

    def __init__(self, hidden: int, joint_size: int, vocab_size: int, s_range: int = 5, simple_loss_scale: float = 0.5,
                 pruned_loss_scale: float = 1.0, lm_only_scale: float = 0.25, am_only_scale: float = 0.0,
                 topology: str = "standard"):
        super().__init__()
        J, V, S = int(joint_size), int(vocab_size), int(s_range)
        if J % 64 != 0 or not 64 <= J <= MAX_JOINT_SIZE:
            raise ValueError(f"PrunedJointLoss: the joint size must be a multiple of 64 in 64 ... {MAX_JOINT_SIZE}, got {joint_size}")
        if not 2 <= V <= MAX_ALPHABET_SIZE:
            raise ValueError(f"PrunedJointLoss: the vocabulary size must be in 2 ... {MAX_ALPHABET_SIZE}, got {vocab_size}")
        if not 1 <= S <= MAX_S_RANGE:
            raise ValueError(f"PrunedJointLoss: s_range must be in 1 ... {MAX_S_RANGE}, got {s_range!r}")
        self.s_range = S
        self.simple_loss_scale = float(simple_loss_scale)
        self.pruned_loss_scale = float(pruned_loss_scale)
        self.lm_only_scale, self.am_only_scale = check_simple_scales(lm_only_scale, am_only_scale)
        self.topology = check_topology(topology)
        self.am_head = nn.Linear(hidden, V)
        self.lm_head = nn.Linear(hidden, V)
        self.last_simple_costs = self.last_pruned_costs = self.last_s_begin = None

    def forward(self, joint, enc, pred, labels, input_lengths, label_lengths):
        """Per-utterance objective [B] from the model's JointLoss `joint`, enc [B, T, H] and pred [B, U, H]; `blank_label` and
        `fastemit_lambda` are the joint's."""
        enc_proj = enc @ joint.W1 + joint.b1
        pred_proj = pred @ joint.W1
        simple, pruned, s_begin = rnnt_loss_two_pass_fused(
            self.am_head(enc), self.lm_head(pred), enc_proj, pred_proj, joint.W2, joint.b2, labels, input_lengths, label_lengths,
            self.s_range, blank_label=joint.blank_label, lm_only_scale=self.lm_only_scale, am_only_scale=self.am_only_scale,
            fastemit_lambda=joint.fastemit_lambda, topology=self.topology, ordered_ranges=True)
        self.last_simple_costs, self.last_pruned_costs, self.last_s_begin = simple.detach(), pruned.detach(), s_begin
        return self.simple_loss_scale * simple + self.pruned_loss_scale * pruned
