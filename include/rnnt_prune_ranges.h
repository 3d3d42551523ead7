/* rnnt_prune_ranges.h -- the band positions of the pruned transducer loss, with a DEFINED order of additions.  An extension of
 * include/rnnt.h.
 *
 * include/rnnt.h and libwarprnnt.so are the library's base interface and stay as they are.  The entry point declared here is what
 * libwarprnnt_pruneranges.so exports, and all it exports (csrc/rnnt_prune_ranges.map).  The extension library is self-contained:
 * its own kernels, no workspace; it shares nothing with the other libraries but the types of rnnt.h.
 */
#ifndef RNNT_PRUNE_RANGES_H
#define RNNT_PRUNE_RANGES_H

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build-only extension (no upstream counterpart; the idea is k2's get_rnnt_prune_ranges): where each frame's band of S = s_range
 * symbols begins, from the per-cell occupancies of a first pass (compute_rnnt_loss_simple, include/rnnt_simple.h).  Its result is
 * the s_begin of compute_rnnt_loss_pruned (include/rnnt_pruned.h) and compute_rnnt_joint_loss_pruned (include/rnnt_pruned_joint.h).
 *
 * INPUTS.
 *   occupancy  float32 [minibatch, options.maxT, options.maxU], contiguous;
 *   input_lengths, label_lengths  int32 [minibatch];
 *   s_begin    int32 [minibatch, options.maxT]: EVERY element is written.
 *
 * THE RULE (it is the definition; pruning.py prune_ranges(..., ordered=True) mirrors it on the CPU and tests/prune_ranges_cases.py
 * restates it in loops).  Per utterance b: T_b = input_lengths[b] clamped into [1, maxT], L_b = label_lengths[b] clamped into
 * [0, maxU - 1], hi = max(0, L_b + 1 - S).
 *   1. For each frame t < T_b:  w(s0) = ((occ[t, s0] + occ[t, s0 + 1]) + ...) + occ[t, s0 + S - 1]  for s0 = 0 ... hi: the terms
 *      widened to float64 and added in INCREASING s, starting from the first term.  raw[t] is the LOWEST s0 whose w is largest:
 *      going over s0 = 0 ... hi, a candidate replaces the best so far only when w > best; the best starts at -inf with s0 = 0, so
 *      a NaN sum never wins (and a row of NaN sums answers 0).  When hi = 0 the answer is 0 and nothing is read.
 *   2. raw[0] = 0, then raw[T_b - 1] = hi.
 *   3. A running maximum forwards: the result is non-decreasing.
 *   4. Backwards over t = T_b - 2 ... 1:  sb[t] = max(sb[t], sb[t + 1] - (S - 1)), so consecutive bands overlap.
 *   5. The frames t >= T_b hold hi.
 * Steps 2 - 5 are those of prune_ranges(..., ordered=False); step 1's order of additions is what that route leaves to torch.  A
 * running sum (add the entering term, subtract the leaving one) is NOT this rule: it gives other bits on exactly the peaked rows
 * -- one occupancy near 1, its neighbours at 1e-11 ... 1e-20 -- on which the order decides which of two windows wins.
 *
 * No element of occupancy outside t < T_b, u <= L_b is read (a window that begins in [0, hi] ends at s0 + S - 1 <= L_b when
 * hi > 0): those elements may hold anything, NaN included.  An utterance's result does not depend on the batch around it.  Two
 * launches on options.stream (the windows, then steps 2 - 5 in place on s_begin), no workspace, no memset, no atomics: two calls
 * on the same input give the same bits.
 *
 * RNNT_STATUS_INVALID_VALUE before anything is enqueued: a NULL pointer; minibatch < 1 or maxT < 1; maxU outside [1, 8192];
 * s_range outside [1, 64]; minibatch * maxT * maxU >= 2^31; options.loc != RNNT_GPU (a device-only library). */
RNNT_API rnntStatus_t compute_rnnt_prune_ranges(const float *occupancy, const int *input_lengths, const int *label_lengths,
                                                int minibatch, int s_range, int *s_begin, rnntOptions options);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_PRUNE_RANGES_H */
