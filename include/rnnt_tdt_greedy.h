/* rnnt_tdt_greedy.h -- batched greedy decoding of a token-and-duration (TDT) transducer: an extension of include/rnnt.h.
 *
 * include/rnnt.h and libwarprnnt.so, include/rnnt_tdt.h and libwarprnnt_tdt.so stay as they are.  The three entry points declared
 * here are what libwarprnnt_tdtgreedy.so exports, and all it exports; no other library holds anything of them.  The library links
 * the base library's kernel objects (the greedy decoder's prepare path and the per-hypothesis joint run unchanged) beside its own
 * step and update kernels, and works on a workspace of its own.
 */
#ifndef RNNT_TDT_GREEDY_H
#define RNNT_TDT_GREEDY_H

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build-only extension (no upstream counterpart): batched GREEDY DECODING of the token-and-duration transducer (Xu et al. 2023) --
 * the decoder of the model compute_rnnt_loss_tdt (include/rnnt_tdt.h) trains, in the form of compute_rnnt_greedy_begin / _step
 * (include/rnnt.h): the caller steps the prediction network; the library evaluates the joint for one lattice cell per hypothesis --
 * its current frame against its prediction-network output -- and does both argmaxes, the two log-softmaxes of the decision and the
 * state update in the same pass, without writing logits.
 *
 * V = alphabet_size tokens (blank included), D = num_durations, R = V + D.
 *   W2 [joint_size, R], b2 [R]   device f32.  The first V columns are the token head, the last D the duration head: the row layout
 *                 of compute_rnnt_loss_tdt's acts.
 *   durations     HOST int [D], read during begin only, under the rule of include/rnnt_tdt.h: strictly increasing, durations[0] in
 *                 {0, 1}, some d > 0 present, 1 <= D <= 8, durations[D-1] <= 8.  The set reaches the device as kernel arguments
 *                 (no host-to-device copy, no memset) and stays in the workspace: the steps take num_durations alone.
 *   max_per_frame >= 1: non-blank symbols emitted in a row on one frame at most.  With a duration 0 in the set an uncapped decoder
 *                 need not terminate, so there is no "no cap" value here.
 *   enc_proj, pred_proj, frame_lengths, max_symbols, hyps, hyp_lengths, scores, emitted, all_done, options: exactly as for
 *                 compute_rnnt_greedy_begin / _step -- lengths clamped into the tensor (frame_lengths into [0, maxT], a negative
 *                 max_symbols = 0, NULL = no limit beyond max_hyp_len); a hypothesis that fills max_hyp_len symbols below its
 *                 max_symbols is PAUSED (all_done = 2) until steps with a larger max_hyp_len resume it; a hypothesis that is done
 *                 (or paused) reads nothing and writes only hyp_lengths / scores (unchanged) and emitted = -1.
 *   hyp_frames    device i32 [minibatch, max_hyp_len], hyp_logp device f32 [minibatch, max_hyp_len]: both given or both NULL.  Per
 *                 token, at its position in hyps: the frame of the decision that emitted it, and the token log-probability plus
 *                 the duration log-probability of that decision.  Nothing else is written to them.
 *   logit_stats   device f32 [minibatch, 4] or NULL: {max token logit, token logsumexp, max duration logit, duration logsumexp} of
 *                 this step's joint, written for the hypotheses that ran.
 *
 * compute_rnnt_tdt_greedy_begin (once per decode) builds what compute_rnnt_greedy_begin builds, over all R columns, resets every
 * hypothesis (frame 0, no symbols, score 0; done when frame_lengths[b] or max_symbols[b] is 0) and stores the duration set.
 * The workspace then holds everything the steps need.
 * compute_rnnt_tdt_greedy_step (once per decode step), for every hypothesis b that is not done, with
 * logits = tanh(enc_proj[b, t_b] + pred_proj[b]) @ W2 + b2  (R of them), t = t_b, n = n_b, nf = symbols emitted on this frame so far:
 *   k = argmax_{v < V} logits[v]          (lowest index on ties)
 *   i = argmax_{j < D} logits[V + j]      (lowest index on ties), d = durations[i]
 *   scores[b] += (logits[k] - lse_tokens) + (logits[V + i] - lse_durations)      (f64 sum inside; the sigma of the loss plays no
 *                                                                                  part at decode time)
 *   k != blank:  hyps[b, n] = k, n += 1, nf += 1, emitted[b] = k;  if d == 0 and nf >= max_per_frame: d = 1
 *   k == blank:  emitted[b] = -1;                                   if d == 0: d = 1
 *   if d > 0: nf = 0
 *   t += d                                 (the last jump may pass T_b)
 *   done when t >= T_b or n >= max_symbols[b]
 * A head with no finite logit has no argmax: the token head then counts as the blank and the duration head as d = 1; the score
 * becomes NaN (as compute_rnnt_greedy_step's does).
 *
 * Numerics: for a hypothesis, both (argmax, max logit) pairs are bitwise those of compute_rnnt_joint_logits called with
 * alphabet_size = V + D for that hypothesis alone (minibatch = maxT = maxU = 1, the same joint_dtype): the per-hypothesis joint
 * of the greedy and beam decoders, unchanged, route switches per hypothesis included.  The two logsumexps: f32 partial sums per
 * 32-column chunk, combined in float64, as the greedy decoder forms its one.  Single stream, no atomics, no memset: two decodes
 * of the same input give the same bits, and a hypothesis's result does not depend on the batch around it.
 * Shapes: every (joint_dtype, joint_size, R) that compute_rnnt_greedy_step takes with alphabet_size = R.  joint_dtype carries no
 * flag bits.  workspace: get_rnnt_tdt_greedy_workspace_size(maxT, minibatch, ...) bytes, 256-byte aligned, owned by one decode
 * from its begin to its last step; it may hold anything on entry.  It is the greedy workspace at alphabet_size = R followed by
 * the duration head's partial results and the duration set.  No entry point synchronises the host.
 * RNNT_STATUS_INVALID_VALUE before anything is enqueued: every case compute_rnnt_greedy_begin / _step reject (a NULL required
 * pointer, a non-positive size, a joint_dtype other than 0 / 1, options.loc != RNNT_GPU, options.batch_first == false, maxT or maxU
 * < 1, a workspace that is not 256-byte aligned, minibatch * maxT * joint_size >= 2^31, max_hyp_len < 1 or max_hyp_len * minibatch
 * >= 2^31); a durations array that breaks the rule above (or is NULL); num_durations outside [1, 8]; alphabet_size < 2; the blank
 * outside [0, alphabet_size); max_per_frame < 1; exactly one of hyp_frames / hyp_logp NULL; hyps, hyp_frames or hyp_logp not
 * 4-byte aligned; a (joint_dtype, joint_size, R) the greedy decoder does not take.  get_rnnt_tdt_greedy_workspace_size returns it
 * for a NULL size_bytes and for the same shape limits. */
RNNT_API rnntStatus_t get_rnnt_tdt_greedy_workspace_size(int maxT, int minibatch, int joint_size, int alphabet_size,
                                                         int num_durations, int joint_dtype, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_tdt_greedy_begin(const float *enc_proj, const int *frame_lengths, const int *max_symbols,
                                                    const float *W2, const float *b2, int joint_size, int alphabet_size,
                                                    const int *durations, int num_durations, int minibatch, int max_per_frame,
                                                    int joint_dtype, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_tdt_greedy_step(const float *pred_proj, int *hyps, int *hyp_frames, float *hyp_logp,
                                                   int max_hyp_len, int *hyp_lengths, float *scores, int *emitted, int *all_done,
                                                   float *logit_stats, int joint_size, int alphabet_size, int num_durations,
                                                   int minibatch, int joint_dtype, void *workspace, rnntOptions options);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_TDT_GREEDY_H */
