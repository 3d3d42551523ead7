/* rnnt_simple.h -- the SIMPLE transducer loss: an additive joiner, the first pass of the pruned loss.  An extension of
 * include/rnnt.h.
 *
 * include/rnnt.h and libwarprnnt.so are the library's base interface and stay as they are.  The two entry points declared here
 * are what libwarprnnt_simple.so exports, and all it exports (csrc/rnnt_simple.map).  The extension library is self-contained: its
 * own kernels, its own workspace; it shares nothing with the other libraries but the types of rnnt.h.
 */
#ifndef RNNT_SIMPLE_H
#define RNNT_SIMPLE_H

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RNNT_SIMPLE_STANDARD 0 /* the lattice of compute_rnnt_loss: a label edge stays on its frame */
#define RNNT_SIMPLE_MODIFIED 1 /* the lattice of compute_rnnt_loss_modified (include/rnnt_modified.h): one symbol per frame */

/* Build-only extension (no upstream counterpart; the idea is k2's rnnt_loss_simple / rnnt_loss_smoothed): loss, gradients and
 * per-cell occupancies of the joiner logit(t, u, v) = am[t, v] + lm[u, v].  It needs am and lm alone -- the [B, T, U, V] tensor
 * is never formed, in memory or in a gradient -- and its occupancies are what prune_ranges (pruning.py) turns into the band of
 * compute_rnnt_loss_pruned (include/rnnt_pruned.h).
 *
 * INPUTS.  Per utterance b: T = T_b = input_lengths[b] frames, L = L_b = label_lengths[b] labels y_0 ... y_{L-1}.
 *   am  float32 [minibatch, maxT, V], contiguous;  lm  float32 [minibatch, maxU, V], contiguous, maxU = options.maxU;
 *   options.maxU - 1 is the row stride of flat_labels, as everywhere.
 * Cell (t, u) is PRESENT iff t < T and u <= L.  The rows am[b, t >= T_b] and lm[b, u > L_b] are never read.
 *
 * EDGE LOG-PROBABILITIES.  With a = am_only_scale, l = lm_only_scale, w = 1 - a - l; each of a, l and a + l (the float32 sum)
 * finite and in [0, 1]:
 *   Z(t,u) = ln sum_v exp(am[t,v] + lm[u,v]),  Za(t) = ln sum_v exp(am[t,v]),  Zl(u) = ln sum_v exp(lm[u,v])
 *   lp(t,u,v) = w (am[t,v] + lm[u,v] - Z(t,u)) + a (am[t,v] - Za(t)) + l (lm[u,v] - Zl(u))
 *   lpb(t,u) = lp(t,u,blank),  lpl(t,u) = lp(t,u,y_u)   (there is no lpl for u = L)
 * This is the same idea as k2's smoothed interpolation WITHOUT its batch-coupled unigram term (an utterance's results do not
 * depend on the batch around it) and it is NOT bit-compatible with k2: the rule above is the definition.
 *
 * LATTICES.  topology = RNNT_SIMPLE_STANDARD or RNNT_SIMPLE_MODIFIED: exactly the recurrences, the end conditions and the
 * e_b, e_l of include/rnnt_pruned.h with every cell of the full lattice present:
 *   standard:  alpha(0,0) = 0;  alpha(t,u) = logaddexp(alpha(t-1,u) + lpb(t-1,u), alpha(t,u-1) + lpl(t,u-1))
 *              ln P = alpha(T-1,L) + lpb(T-1,L);  beta(T-1,L) = lpb(T-1,L)
 *              beta(t,u) = logaddexp(lpb(t,u) + beta(t+1,u), lpl(t,u) + beta(t,u+1))
 *   modified:  alpha(0,0) = 0;  alpha(t,u) = logaddexp(alpha(t-1,u) + lpb(t-1,u), alpha(t-1,u-1) + lpl(t-1,u-1));  ln P = alpha(T,L)
 *              beta(T,L) = 0, every other beta(T,u) = -inf;  beta(t,u) = logaddexp(lpb(t,u) + beta(t+1,u), lpl(t,u) + beta(t+1,u+1))
 *   e_b = exp(alpha(t,u) + lpb(t,u) + beta(blank target) - ln P)      (= exp(alpha + lpb - ln P) at the standard (T-1,L))
 *   e_l = exp(alpha(t,u) + lpl(t,u) + beta(label target) - ln P)      (0 for u = L)
 * A modified utterance with L > T has no path: that is legitimate data, its cost is +inf, its gradients and its occupancy are
 * exact zeros, never NaN.
 *
 * OUTPUTS.  Each nullable as stated; EVERY element of a given buffer is written.  With occ = e_b + e_l, sj = exp(am + lm - Z),
 * sa = exp(am - Za), sl = exp(lm - Zl), eps(t,u,v) = [v == blank] e_b + [u < L and v == y_u] e_l, cs = cost_scale[b] (NULL: 1)
 * and the sums over the present cells:
 *   costs[b]         = -ln P
 *   occupancy[b,t,u] = occ            float32 [minibatch, maxT, maxU]; 0 on absent cells; what prune_ranges takes
 *   grad_am[b,t,v]   = cs (w sum_u occ(t,u) sj(t,u,v) + a sa(t,v) sum_u occ(t,u) - (w + a) sum_u eps(t,u,v))
 *   grad_lm[b,u,v]   = cs (w sum_t occ(t,u) sj(t,u,v) + l sl(u,v) sum_t occ(t,u) - (w + l) sum_t eps(t,u,v))
 * -- d costs[b] / d am and d lm, scaled.  The padded rows of grad_am and grad_lm are exact zeros.
 * Out-of-range lengths and labels follow the rule of compute_rnnt_loss: T_b is clamped into [1, maxT], L_b into [0, maxU - 1],
 * labels into [0, V); an utterance with an out-of-range length has a NaN cost and NaN occupancies and gradients on its clamped
 * lattice (zeros beside it).
 *
 * ARGUMENTS.
 *   grad_am, grad_lm     given together or not at all;
 *   costs != NULL        the forward (it writes occupancy if that is given), then the gradient pass if the gradients are given;
 *   costs == NULL        the gradient pass alone, from the workspace a forward left: any number of times, with any cost_scale.
 *                        occupancy, if given, is written again from that workspace.  The caller MUST pass the topology and
 *                        the two scales of that forward: the gradient kernels take w, a and l from the call they run in, the
 *                        workspace does not record them, and nothing checks that they agree.
 *   cost_scale           device f32 [minibatch] or NULL (= 1); the costs do not depend on it.
 *   workspace            >= get_rnnt_simple_workspace_size() bytes, 256-byte aligned.  Its size is a function of maxT, maxU and
 *                        minibatch alone -- never of V.  It may hold anything on entry.
 * RNNT_STATUS_INVALID_VALUE before anything is enqueued: a NULL required pointer; nothing to compute (costs, occupancy and the
 * gradients all NULL); exactly one of grad_am, grad_lm; alphabet_size < 2; the blank outside [0, alphabet_size); a topology that
 * is not 0 or 1; maxU outside [1, 8192]; minibatch * maxT * maxU >= 2^31; a workspace that is not 256-byte aligned; a scale
 * outside the rule above; and, when the gradients are requested, a vocabulary so large that the gradient passes' grid does not
 * fit: minibatch * ceil(alphabet_size / 16) * ((maxT + maxU + 30) / 16 + 1) >= 2^31 (integer division; at B32 T600 U150 that is
 * a vocabulary beyond 22 million symbols).
 *
 * NUMERICS.  The rule of rnnt_modified.h and rnnt_pruned.h: the recurrences are carried in float64, the log(1 + e^-|d|) term of
 * a log-add on the float32 units, alpha and beta are STORED as float64.  Z, sj and the two gradient reductions are evaluated
 * directly, as exp(am + lm - m) with the cell's own maximum m, so that every exponential is at most 1: a product of separately
 * shifted exp(am - max am) exp(lm - max lm) underflows to a zero sum when am and lm peak at different symbols, and is not used.
 * The bars of the project hold against the float64 restatement (tests/simple_cases.py): costs within 1e-4 max(1, |cost|),
 * occupancy within 1e-4, gradients within 1e-4 |cost_scale| max(1, max |reference|) per utterance
 * (tests/test_simple_loss_gpu.py).  FastEmit is not part of this op: the second pass (rnnt_pruned.h) has it.
 * Single stream, no memset, no atomics: two calls on the same input give the same bits, and an utterance's results do not depend
 * on the batch around it. */
RNNT_API rnntStatus_t get_rnnt_simple_workspace_size(int maxT, int maxU, int minibatch, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_loss_simple(const float *am, const float *lm, float *grad_am, float *grad_lm, float *occupancy,
                                      const int *flat_labels, const int *label_lengths, const int *input_lengths,
                                      const float *cost_scale, int alphabet_size, int minibatch, int topology,
                                      float lm_only_scale, float am_only_scale, float *costs, void *workspace,
                                      rnntOptions options);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_SIMPLE_H */
