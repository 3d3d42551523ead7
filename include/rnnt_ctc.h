/* rnnt_ctc.h -- a CTC loss and a greedy CTC decoder for the auxiliary CTC head of a hybrid transducer + CTC model: an extension of
 * include/rnnt.h.
 *
 * include/rnnt.h and libwarprnnt.so are the library's base interface and stay as they are.  The three entry points declared here
 * are what libwarprnnt_ctc.so exports, and all it exports; libwarprnnt.so holds nothing of them.  The extension library is
 * self-contained: it works on a workspace of its own and shares nothing with the base library but the types of rnnt.h.
 */
#ifndef RNNT_CTC_H
#define RNNT_CTC_H

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build-only extension (no upstream counterpart): the CTC loss of the encoder's auxiliary head, with the conventions of
 * compute_rnnt_loss for the blank, the lengths and infinite costs.
 *   acts         device f32 [minibatch, maxT, alphabet_size], raw logits; the log-softmax is fused
 *   flat_labels  device i32 [minibatch, maxU - 1]: options.maxU - 1 is the row stride and the largest L
 * Per utterance, T = T_b frames, L = L_b labels y_0 ... y_{L-1}, lp(t,v) = log_softmax(acts[b,t,:])[v], states s = 0 ... 2L with the
 * symbol z_s: the blank for even s, y_{(s-1)/2} for odd s:
 *   alpha(0,0) = lp(0,blank), alpha(0,1) = lp(0,y_0) (L >= 1), every other alpha(0,s) = -inf
 *   alpha(t,s) = lp(t,z_s) + logsumexp(alpha(t-1,s), alpha(t-1,s-1) [s >= 1], alpha(t-1,s-2) [s odd, s >= 3, z_s != z_{s-2}])
 *   ln P = logaddexp(alpha(T-1,2L), alpha(T-1,2L-1))  (the first term alone for L = 0),  costs[b] = -ln P
 *   beta(T-1,2L) = lp(T-1,blank), beta(T-1,2L-1) = lp(T-1,y_{L-1}) (L >= 1), every other beta(T-1,s) = -inf
 *   beta(t,s) = lp(t,z_s) + logsumexp(beta(t+1,s), beta(t+1,s+1) [s < 2L], beta(t+1,s+2) [s odd, s + 2 <= 2L, z_{s+2} != z_s])
 *   occ(t,s) = exp(alpha(t,s) + beta(t,s) - lp(t,z_s) - ln P)
 *   grads[b,t,v] = cost_scale[b] (softmax(acts[b,t,:])[v] - sum over {s : z_s = v} of occ(t,s))
 * Every element of grads is written; frames t >= T_b get exact zeros and their logits are not read.
 * An utterance with no path (T_b < L_b + the number of adjacent equal labels) is legitimate data: its cost is +inf and all of its
 * gradients are exact zeros, never NaN.
 * Out-of-range lengths (T_b outside [1, maxT], L_b outside [0, maxU - 1]) are clamped, and that utterance's cost and the gradients
 * of its clamped frames are NaN, as in compute_rnnt_loss.  Labels are clamped into [0, alphabet_size); a label (of the L_b read)
 * that equals the blank marks the utterance invalid in the same way.  This is decided on the device: labels are device data.
 * Numerics.  The sweeps take T_b serial steps with all 2 L_b + 1 states in flight, alpha and beta side by side in one launch.  The
 * recurrence is carried in float64, the log(1 + e^-|d|) term of a log-add on the float32 units, and alpha / beta are STORED as
 * float64, the rule of rnnt_modified.h for the same reason.  The bars of compute_rnnt_loss hold: costs within 1e-4 max(1, |cost|),
 * gradients within 1e-4 |cost_scale| absolute (tests/test_ctc_gpu.py; measured values in profiles/ctc_notes.md).
 * Every sum has an order fixed by the utterance alone (the sum over the positions of a repeated symbol runs in increasing
 * position): no float atomics, two calls give the same bits, an utterance's results do not depend on the batch around it.
 *   workspace      >= get_rnnt_ctc_workspace_size() bytes, 256-byte aligned, its own layout; it may hold anything on entry.  Its
 *                  size does not depend on alphabet_size.  Limits: maxU in [1, 8192], minibatch * maxT * (2 maxU - 1) < 2^31,
 *                  minibatch * maxT * alphabet_size < 2^31.
 *   grads == NULL  the forward alone;  costs == NULL  the gradient pass alone, from the workspace a forward left (any number of
 *                  times, with any cost_scale);  both: forward then backward on the caller's stream.
 *   cost_scale     device f32 [minibatch] or NULL (= 1).
 * Everything is enqueued on options.stream: no memset, no allocation, no synchronisation.
 * RNNT_STATUS_INVALID_VALUE before anything is enqueued: a NULL required pointer (costs and grads both NULL included),
 * alphabet_size < 2, the blank outside [0, alphabet_size), a shape over the limits, a workspace that is not 256-byte aligned, a
 * pointer that is not 4-byte aligned, options.loc != RNNT_GPU, options.batch_first == false. */
RNNT_API rnntStatus_t get_rnnt_ctc_workspace_size(int maxT, int maxU, int minibatch, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_ctc_loss(const float *acts, float *grads, const int *flat_labels,
                                   const int *label_lengths, const int *input_lengths,
                                   const float *cost_scale, int alphabet_size, int minibatch,
                                   float *costs, void *workspace, rnntOptions options);

/* Greedy (best path) decoding of the same head.  a_t = argmax_v acts[b,t,v], the lowest index on ties; frame t < T_b emits a_t iff
 * a_t != blank and (t == 0 or a_t != a_{t-1}).
 *   acts           device f32 [minibatch, maxT, alphabet_size]; frames t >= T_b are not read
 *   input_lengths  device i32 [minibatch], clamped into [0, maxT]
 *   tokens         device i32 [minibatch, maxT]: the emitted symbols in frame order, then -1 from index lengths[b] on
 *   token_frames   device i32 [minibatch, maxT] or NULL: the frame that emitted each token, then -1
 *   lengths        device i32 [minibatch]
 * options.maxU is not read; there is no workspace.  RNNT_STATUS_INVALID_VALUE before anything is enqueued: a NULL required
 * pointer, a pointer that is not 4-byte aligned, alphabet_size < 2, the blank outside the alphabet, maxT < 1, minibatch < 1,
 * minibatch * maxT * alphabet_size >= 2^31, options.loc != RNNT_GPU, options.batch_first == false. */
RNNT_API rnntStatus_t compute_rnnt_ctc_greedy(const float *acts, const int *input_lengths, int alphabet_size, int minibatch,
                                     int *tokens, int *token_frames, int *lengths, rnntOptions options);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_CTC_H */
