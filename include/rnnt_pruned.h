/* rnnt_pruned.h -- the PRUNED transducer loss: the lattice on a band of S symbols per frame.  An extension of include/rnnt.h.
 *
 * include/rnnt.h and libwarprnnt.so are the library's base interface and stay as they are.  The two entry points declared here
 * are what libwarprnnt_pruned.so exports, and all it exports (csrc/rnnt_pruned.map).  The extension library is self-contained: its
 * own kernels, its own workspace; it shares nothing with the other libraries but the types of rnnt.h.
 */
#ifndef RNNT_PRUNED_H
#define RNNT_PRUNED_H

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RNNT_PRUNED_STANDARD 0 /* the lattice of compute_rnnt_loss: a label edge stays on its frame */
#define RNNT_PRUNED_MODIFIED 1 /* the lattice of compute_rnnt_loss_modified (include/rnnt_modified.h): one symbol per frame */

/* Build-only extension (no upstream counterpart; the idea is k2's pruned RNN-T loss): loss and gradients on logits that exist
 * only on a band of S = s_range symbols per frame, given, per frame, where the band begins.  A cheap first pass of the caller's
 * says where the mass of the lattice is; the joint and this op are then evaluated on B x T x S cells instead of B x T x U.
 *
 * PRESENCE OF CELLS.  Per utterance b: T = T_b = input_lengths[b] frames, L = L_b = label_lengths[b] labels y_0 ... y_{L-1},
 * the band width S with 1 <= S <= 64, and sb[t] = s_begin[b, t], a device int32 [minibatch, maxT].
 *   acts  float32 [minibatch, maxT, S, V], contiguous;  acts[b, t, s, :] holds the logits of lattice cell (t, u), u = sb[t] + s.
 * A cell is PRESENT iff 0 <= t < T, 0 <= u <= L and 0 <= s < S.  Every other element of the tensor is ABSENT: padded frames,
 * u > L, u < 0, and anything an arbitrary sb value points at.  Absent cells have no outgoing edges and exact-zero gradients;
 * their logits are never read.  lpb(t,u) and lpl(t,u) are the log-softmax of a present cell's logits at the blank and at y_u
 * (there is no lpl for u = L).
 * ANY int32 is a legal s_begin value: u is computed so that it cannot overflow, and nothing about monotonicity is assumed.  A
 * band that does not connect (0,0) to the end is legitimate data (as L > T is in rnnt_modified.h): its cost is +inf and all of
 * its gradients are exact zeros, never NaN.
 *
 * STANDARD TOPOLOGY (topology = RNNT_PRUNED_STANDARD, the lattice of compute_rnnt_loss):
 *   alpha(0,0) = 0
 *   alpha(t,u) = logaddexp(alpha(t-1,u) + lpb(t-1,u), alpha(t,u-1) + lpl(t,u-1))
 *   ln P = alpha(T-1,L) + lpb(T-1,L)
 *   beta(T-1,L) = lpb(T-1,L)
 *   beta(t,u) = logaddexp(lpb(t,u) + beta(t+1,u), lpl(t,u) + beta(t,u+1))
 *   e_b = exp(alpha(t,u) + lpb(t,u) + beta(t+1,u) - ln P)      (= exp(alpha + lpb - ln P) at (T-1,L))
 *   e_l = exp(alpha(t,u) + lpl(t,u) + beta(t,u+1) - ln P)
 * All of it runs over present cells only: a term whose source or target cell is absent is -inf (e_b, e_l: 0).
 *
 * MODIFIED TOPOLOGY (topology = RNNT_PRUNED_MODIFIED): exactly the recurrence, the end condition and the occupancies of
 * include/rnnt_modified.h, with the same presence rule -- nodes (t, u) with 0 <= t <= T:
 *   alpha(0,0) = 0
 *   alpha(t,u) = logaddexp(alpha(t-1,u) + lpb(t-1,u), alpha(t-1,u-1) + lpl(t-1,u-1))
 *   ln P = alpha(T,L)          (no final blank; row T has no cells, it is the end node (T, L) alone)
 *   beta(T,L) = 0, every other beta(T,u) = -inf
 *   beta(t,u) = logaddexp(lpb(t,u) + beta(t+1,u), lpl(t,u) + beta(t+1,u+1))
 *   e_b = exp(alpha(t,u) + lpb(t,u) + beta(t+1,u) - ln P)
 *   e_l = exp(alpha(t,u) + lpl(t,u) + beta(t+1,u+1) - ln P)
 *
 * BOTH TOPOLOGIES.
 *   costs[b] = -ln P
 *   occ = e_b + e_l
 *   grads[b,t,s,v] = cost_scale[b] * ((occ + lambda e_l) softmax(acts[b,t,s,:])[v] - [v == blank] e_b - [v == y_u] (1 + lambda) e_l)
 * -- FastEmit's form of compute_rnnt_loss_fastemit; the costs do not depend on lambda.  Every element of grads is written.
 * Out-of-range lengths and labels follow the rule of compute_rnnt_loss: T_b is clamped into [1, maxT], L_b into [0, maxU - 1],
 * labels into [0, V); an utterance with an out-of-range length has a NaN cost and NaN gradients on the present cells of its
 * clamped lattice.
 *
 * ARGUMENTS.
 *   options.maxT         acts.shape[1];  options.maxU - 1 is the row stride of flat_labels, as everywhere.
 *   grads == NULL        the forward alone;
 *   costs == NULL        the gradient pass alone, from the workspace a forward left: any number of times, with any
 *                        cost_scale / fastemit_lambda;  both given: forward then gradient pass on the caller's stream.
 *   cost_scale           device f32 [minibatch] or NULL (= 1).  fastemit_lambda finite and in [0, 1].
 *   workspace            >= get_rnnt_pruned_workspace_size() bytes, 256-byte aligned.  Its size is a function of maxT, s_range
 *                        and minibatch alone -- never of V or of maxU.  It may hold anything on entry.
 * RNNT_STATUS_INVALID_VALUE before anything is enqueued: a NULL required pointer (costs and grads both NULL included),
 * alphabet_size < 2, the blank outside [0, alphabet_size), s_range outside [1, 64], a topology that is not 0 or 1, maxU outside
 * [1, 8192], minibatch * maxT * s_range >= 2^31, a workspace that is not 256-byte aligned, a fastemit_lambda that is not finite or
 * not in [0, 1].
 *
 * NUMERICS.  The rule of include/rnnt.h, as rnnt_modified.h follows it: the recurrence is carried in float64, the
 * log(1 + e^-|d|) term of a log-add on the float32 units; alpha and the edge terms of beta are STORED as float64 (a band is
 * narrow: this costs nothing that matters).  The bars of compute_rnnt_loss hold against the float64 restatement
 * (tests/pruned_cases.py): costs within 1e-4 max(1, |cost|), gradients within 1e-4 |cost_scale| absolute
 * (tests/test_pruned_loss_gpu.py).
 * Single stream, no memset, no atomics; an utterance's results do not depend on the batch around it. */
RNNT_API rnntStatus_t get_rnnt_pruned_workspace_size(int maxT, int s_range, int minibatch, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_loss_pruned(const float *acts, float *grads, const int *s_begin, const int *flat_labels,
                                      const int *label_lengths, const int *input_lengths, const float *cost_scale,
                                      int alphabet_size, int minibatch, int s_range, int topology, float *costs,
                                      void *workspace, rnntOptions options, float fastemit_lambda);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_PRUNED_H */
