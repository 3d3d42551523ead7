/* rnnt_pruned_joint.h -- the FUSED JOINT ON THE PRUNED BAND: costs and gradients of the pruned transducer loss straight from the
 * joint network's projections.  An extension of include/rnnt.h and include/rnnt_pruned.h.
 *
 * include/rnnt.h and libwarprnnt.so are the library's base interface and stay as they are, and so do include/rnnt_pruned.h and
 * libwarprnnt_pruned.so.  The two entry points declared here are what libwarprnnt_prunedjoint.so exports, and all it exports
 * (csrc/rnnt_pruned_joint.map).  The extension library is self-contained: its own kernels and workspace, and its own copy of the
 * pruned loss's lattice sweeps.
 */
#ifndef RNNT_PRUNED_JOINT_H
#define RNNT_PRUNED_JOINT_H

#include "rnnt_pruned.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build-only extension (no upstream counterpart): compute_rnnt_loss_pruned (include/rnnt_pruned.h) with the joint network inside.
 * Neither the band's logits [B, T, S, V] nor the gathered prediction rows [B, T, S, J] exist in memory, in either pass.
 *
 * LOGITS.  With B = minibatch, maxT = options.maxT, maxU = options.maxU, J = joint_size, V = alphabet_size, S = s_range:
 *   enc_proj   device f32 [B, maxT, J]     pred_proj  device f32 [B, maxU, J]     W2  device f32 [J, V]     b2  device f32 [V]
 *   logits(b, t, s, :) = tanh(enc_proj[b, t, :] + pred_proj[b, u, :]) @ W2 + b2,    u = s_begin[b, t] + s
 * -- the joint of compute_rnnt_joint_loss (include/rnnt.h) on the band of rnnt_pruned.h.  They are evaluated for PRESENT cells
 * only.  An ABSENT slot reads NO row of pred_proj and no row of enc_proj (prune_joint_inputs of the Python package clamps the row
 * index instead; here the range test is made first and no address is formed behind a failed one): rows of pred_proj beyond
 * L_b and rows of enc_proj beyond T_b may hold anything, NaN included.
 *
 * PRESENCE AND EVERYTHING AFTER THE LOGITS are exactly include/rnnt_pruned.h, by reference: the presence rule (t < T_b,
 * 0 <= u <= L_b, u formed in 64 bits, any int32 legal in s_begin, nothing assumed about monotonicity), both topologies
 * (RNNT_PRUNED_STANDARD, RNNT_PRUNED_MODIFIED), the recurrences, FastEmit's gradient form, cost_scale, the clamping of
 * out-of-range lengths and labels, and a band that does not connect: cost +inf and exact-zero gradients.
 * With dlogits(b, t, s, :) the `grads` of rnnt_pruned.h (cost_scale and fastemit_lambda applied, zero on absent slots):
 *   dz(b, t, s, :)    = (dlogits(b, t, s, :) @ W2^T) (1 - h^2),     h = tanh(enc_proj[b, t] + pred_proj[b, u])
 *   d_enc_proj[b, t]  = sum over s of dz(b, t, s)                   in slot order; exact zeros for t >= T_b
 *   d_pred_proj[b, u] = sum over the present slots (t, s) with s_begin[b, t] + s = u of dz(b, t, s), in frame order; exact zeros
 *                       for rows no present cell points at, u > L_b included
 *   dW2 = sum over present slots of h^T dlogits,     db2 = sum over present slots of dlogits
 * -- gradients of sum_b cost_scale[b] cost_b.  The four are all given or all NULL; each is fully overwritten.  An utterance with
 * an out-of-range length has a NaN cost, NaN in the rows of d_enc_proj / d_pred_proj its clamped lattice's present cells touch,
 * and makes dW2 and db2 NaN (they sum over the batch); a band that does not connect contributes zeros everywhere.
 *
 * ARGUMENTS (the NULL conventions of compute_rnnt_loss_pruned).
 *   gradients NULL       the forward alone;
 *   costs == NULL        the gradient pass alone, from the workspace a forward with the same inputs left: any number of times,
 *                        with any cost_scale / fastemit_lambda;  both given: forward, then the gradient pass.
 *   cost_scale           device f32 [minibatch] or NULL (= 1).  fastemit_lambda finite and in [0, 1].
 *   workspace            >= get_rnnt_pruned_joint_workspace_size() bytes, 256-byte aligned.  Its size is a function of maxT,
 *                        s_range, minibatch and joint_size alone -- never of V or of maxU.  It may hold anything on entry.
 *                        It holds per-slot scalars (rnnt_pruned.h's lattice arrays and the low part of the softmax
 *                        denominator), one per-slot [J] array (dz) and a fixed J x 8192 block of partial sums for dW2;
 *                        nothing of size B T S V.
 * DOMAIN.  RNNT_STATUS_INVALID_VALUE before anything is enqueued outside it: a NULL required pointer (costs and the gradients all
 * NULL included; some gradients given and others not), joint_size not a multiple of 64 in 64 ... 640, alphabet_size outside
 * 2 ... 8192 (EVERY value inside is taken, not only multiples of a tile), the blank outside [0, alphabet_size), s_range outside
 * [1, 64], a topology that is not 0 or 1, maxU outside [1, 8192], minibatch * maxT * s_range >= 2^31, minibatch * maxU >= 2^31,
 * enc_proj / pred_proj / d_enc_proj / d_pred_proj not 16-byte aligned, any other array not 4-byte aligned, a workspace that is
 * not 256-byte aligned, a fastemit_lambda that is not finite or not in [0, 1], options.loc != RNNT_GPU, !options.batch_first.
 *
 * ARITHMETIC.  One arithmetic: the f32-grade products of joint_dtype 0 (include/rnnt.h).  Operands are split into binary16
 * hi + lo parts, a product is hi.hi + lo.hi + hi.lo on the f16 matrix units with f32 accumulation.  W2 enters the products scaled
 * by the power of two that puts max |W2| into [2^13, 2^14), so any finite magnitude is taken (the scale stops at 2^100: below
 * max |W2| = 2^-86 the products keep an absolute error of 2^-124 instead of a relative one); dlogits enter theirs scaled by a
 * power of two as well (2^12 at unit cost_scale for dz; one power of two per batch, from max |cost_scale|, for dW2).  The
 * log-softmax is f32 (online maximum / sum across vocabulary tiles; its denominator is kept as an f32 hi + lo pair for the gradient
 * pass); the lattice keeps rnnt_pruned.h's numerics: float64 carry and storage.  Bars against the float64 restatement
 * (tests/pruned_joint_cases.py): costs and every gradient within 1e-4 max(1, max |reference|), gradients times |cost_scale|
 * (tests/test_pruned_joint_gpu.py).
 *
 * EXECUTION.  Single stream, no memset, no atomics: two identical calls give the same bits; costs, d_enc_proj and d_pred_proj of
 * an utterance do not depend on the batch around it. */
RNNT_API rnntStatus_t get_rnnt_pruned_joint_workspace_size(int maxT, int s_range, int minibatch, int joint_size, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_joint_loss_pruned(const float *enc_proj, const float *pred_proj, const float *W2, const float *b2,
                                            const int *s_begin, const int *flat_labels, const int *label_lengths,
                                            const int *input_lengths, const float *cost_scale, int joint_size, int alphabet_size,
                                            int minibatch, int s_range, int topology, float *costs, float *d_enc_proj,
                                            float *d_pred_proj, float *dW2, float *db2, void *workspace, rnntOptions options,
                                            float fastemit_lambda);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_PRUNED_JOINT_H */
