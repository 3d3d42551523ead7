/* rnnt_tdt_joint.h -- the FUSED TDT JOINT: costs and gradients of the token-and-duration (TDT) transducer loss straight from the
 * joint network's projections.  An extension of include/rnnt.h and include/rnnt_tdt.h.
 *
 * include/rnnt.h and libwarprnnt.so are the library's base interface and stay as they are, and so do include/rnnt_tdt.h and
 * libwarprnnt_tdt.so.  The two entry points declared here are what libwarprnnt_tdtjoint.so exports, and all it exports
 * (csrc/rnnt_tdt_joint.map).  The extension library is self-contained: its own kernels and workspace, and its own copy of the TDT
 * loss's lattice sweeps.
 */
#ifndef RNNT_TDT_JOINT_H
#define RNNT_TDT_JOINT_H

#include "rnnt_tdt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build-only extension (no upstream counterpart): compute_rnnt_loss_tdt (include/rnnt_tdt.h) with the joint network inside.
 * Neither the logits [B, T, U, V + D] nor any per-cell [J] array exists in memory, in either pass.
 *
 * LOGITS.  With B = minibatch, maxT = options.maxT, maxU = options.maxU, J = joint_size, V = alphabet_size, D = num_durations:
 *   enc_proj   device f32 [B, maxT, J]     pred_proj  device f32 [B, maxU, J]     W2  device f32 [J, V + D]     b2  device f32 [V + D]
 *   logits(b, t, u, :) = tanh(enc_proj[b, t, :] + pred_proj[b, u, :]) @ W2 + b2
 * -- the joint of compute_rnnt_joint_loss (include/rnnt.h) with two heads on one W2: the first V columns are the token logits
 * (blank included), the last D the duration logits.  They are evaluated for LIVE cells only (t < T_b, u <= L_b).  A padded cell
 * reads NO row of pred_proj and no row of enc_proj (the liveness test is made first and no address is formed behind a failed
 * one): rows of pred_proj beyond L_b and rows of enc_proj beyond T_b may hold anything, NaN included.
 *
 * EVERYTHING AFTER THE LOGITS is exactly include/rnnt_tdt.h, by reference: the two separate log-softmaxes, sigma on the tokens
 * only, the duration set and its rule (HOST int [D], read during the call), the edge rule and the terminal blank edge that must
 * land exactly on T, the recurrences, cost_scale, the clamping of out-of-range lengths and labels, and an utterance without a
 * path: cost +inf and exact zeros from it in all four gradients.
 * With dlogits(b, t, u, :) the `grads` of rnnt_tdt.h (cost_scale applied, zero on padded cells):
 *   dz(b, t, u, :)    = (dlogits(b, t, u, :) @ W2^T) (1 - h^2),     h = tanh(enc_proj[b, t] + pred_proj[b, u])
 *   d_enc_proj[b, t]  = sum over u of dz(b, t, u)      in column order (32 columns at a time, then those sums in column order);
 *                       exact zeros for t >= T_b
 *   d_pred_proj[b, u] = sum over t of dz(b, t, u)      in frame order (32 frames at a time, then those sums in frame order);
 *                       exact zeros for u > L_b
 *   dW2 = sum over live cells of h^T dlogits,     db2 = sum over live cells of dlogits
 * -- gradients of sum_b cost_scale[b] cost_b.  The four are all given or all NULL; each is fully overwritten.  An utterance with
 * an out-of-range length has a NaN cost, NaN in the rows of d_enc_proj / d_pred_proj its clamped lattice's live cells touch, and
 * makes dW2 and db2 NaN (they sum over the batch); the other utterances' costs, d_enc_proj and d_pred_proj are not affected.
 *
 * ARGUMENTS (the NULL conventions of compute_rnnt_loss_tdt).
 *   gradients NULL       the forward alone;
 *   costs == NULL        the gradient pass alone, from the workspace a forward with the same inputs left: any number of times,
 *                        with any cost_scale; the caller passes the SAME durations and sigma again;
 *   both given           forward, then the gradient pass, on the caller's stream (options.stream).
 *   cost_scale           device f32 [minibatch] or NULL (= 1).  sigma finite and >= 0.
 *   workspace            >= get_rnnt_tdt_joint_workspace_size() bytes, 256-byte aligned.  Its size is a function of maxT, maxU,
 *                        minibatch, num_durations and joint_size alone -- never of V.  It may hold anything on entry.  It holds
 *                        rnnt_tdt.h's lattice arrays, per-cell scalars (the low parts of the two softmax denominators and an
 *                        occupancy record of D + 2 floats), the partial sums of d_enc_proj (one [J] row per frame and 32
 *                        columns) and of d_pred_proj (one [J] row per column and 32 frames), and a fixed J x 8192 block of
 *                        partial sums for dW2; nothing of size B T U V and nothing of size B T U J.
 * DOMAIN.  RNNT_STATUS_INVALID_VALUE before anything is enqueued outside it: a NULL required pointer (costs and the gradients all
 * NULL included; some gradients given and others not), joint_size not a multiple of 64 in 64 ... 640, alphabet_size < 2,
 * alphabet_size + num_durations > 8192 (EVERY value inside is taken, not only multiples of a tile), the blank outside
 * [0, alphabet_size), num_durations outside [1, 8], a durations array that breaks the rule of rnnt_tdt.h, a sigma that is
 * negative or not finite, maxU > 1024, minibatch * maxT * maxU >= 2^31, maxT, maxU or minibatch < 1, enc_proj / pred_proj /
 * d_enc_proj / d_pred_proj not 16-byte aligned, any other array not 4-byte aligned, a workspace that is not 256-byte aligned,
 * options.loc != RNNT_GPU, !options.batch_first.  get_rnnt_tdt_joint_workspace_size returns it for a NULL size_bytes and for
 * the same shape limits.
 *
 * ARITHMETIC.  One arithmetic: the f32-grade products of joint_dtype 0 (include/rnnt.h), as in rnnt_pruned_joint.h.  Operands are
 * split into binary16 hi + lo parts, a product is hi.hi + lo.hi + hi.lo on the f16 matrix units with f32 accumulation.  W2
 * enters the products scaled by the power of two that puts max |W2| into [2^13, 2^14) (the scale stops at 2^100); dlogits enter
 * theirs scaled by a power of two as well (2^12 at unit cost_scale for dz; one power of two per batch, from max |cost_scale|,
 * for dW2).  The two log-softmaxes are f32 (online maximum / sum across tiles of 32 logit columns; each denominator is kept as
 * an f32 hi + lo pair for the gradient pass); the lattice keeps rnnt_tdt.h's numerics: float64 carry and storage.  A tile of
 * 32 cells whose occupancies are all EXACTLY zero is skipped by the gradient pass (its contribution is exactly zero); there is no
 * threshold above zero.  Bars against the float64 restatement (tests/tdt_joint_cases.py): costs and every gradient within
 * 1e-4 max(1, max |reference|), gradients times |cost_scale| (tests/test_tdt_joint_gpu.py).
 *
 * EXECUTION.  Single stream, no memset, no atomics: two identical calls give the same bits; costs, d_enc_proj and d_pred_proj of
 * an utterance do not depend on the batch around it.  Every split of the work (tiles of 32 columns, chunks of 32 frames, the
 * number of dW2 partials) is a function of the shapes alone, never of the device. */
RNNT_API rnntStatus_t get_rnnt_tdt_joint_workspace_size(int maxT, int maxU, int minibatch, int num_durations, int joint_size,
                                                        size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_joint_loss_tdt(const float *enc_proj, const float *pred_proj, const float *W2, const float *b2,
                                                  const int *flat_labels, const int *label_lengths, const int *input_lengths,
                                                  const float *cost_scale, int joint_size, int alphabet_size, const int *durations,
                                                  int num_durations, float sigma, int minibatch, float *costs, float *d_enc_proj,
                                                  float *d_pred_proj, float *dW2, float *db2, void *workspace, rnntOptions options);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_TDT_JOINT_H */
