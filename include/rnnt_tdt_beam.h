/* rnnt_tdt_beam.h -- batched beam search of a token-and-duration (TDT) transducer: an extension of include/rnnt.h.
 *
 * include/rnnt.h and libwarprnnt.so, and every other extension header and library, stay as they are.  The four entry points declared
 * here are what libwarprnnt_tdtbeam.so exports, and all it exports; no other library holds anything of them.  The library links the
 * base library's kernel objects (the greedy decoder's prepare path and the per-hypothesis joint run unchanged) beside its own step,
 * select, begin and results kernels, and works on a workspace of its own.
 */
#ifndef RNNT_TDT_BEAM_H
#define RNNT_TDT_BEAM_H

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build-only extension (no upstream counterpart): batched BEAM SEARCH of the token-and-duration transducer (Xu et al. 2023), the
 * n-best decoder of the model compute_rnnt_loss_tdt (include/rnnt_tdt.h) trains, in the form of compute_rnnt_beam_begin / _step /
 * _results (include/rnnt.h): frame-synchronous, one symbol per frame.  The caller steps the prediction network on minibatch * beam
 * rows and runs maxT steps without a host read; a hypothesis holds at most one token per frame.
 *
 * V = alphabet_size tokens (blank included), D = num_durations, R = V + D.  T_b = frame_lengths[b] clamped into [0, maxT].
 *   W2 [joint_size, R], b2 [R]   device f32: the first V columns are the token head, the last D the duration head.
 *   durations     HOST int [D], read during begin only, under the rule of include/rnnt_tdt.h (strictly increasing, durations[0] in
 *                 {0, 1}, some d > 0, 1 <= D <= 8, durations[D-1] <= 8).  The set reaches the device as kernel arguments (no
 *                 host-to-device copy, no memset) and stays in the workspace.
 *   timed         0 / non-zero, the same in every call of one decode: non-zero keeps per token its frame and duration.
 *
 * THE RULE.  Per utterance the beam holds up to `beam` hypotheses (y, c, s): y a token sequence, c the CURSOR -- the next frame the
 * hypothesis reads -- and s a float64 log score.  The beam starts as [((), 0, 0)].  Per frame t < T_b (every c_i >= t):
 *   1. Hypothesis i is ACTIVE iff c_i == t, else WAITING.  For an active one: logits_i = tanh(enc_proj[b, t] + pred_proj[i]) @ W2
 *      + b2 (R of them, f32), lseT_i the logsumexp of the first V, lseD_i of the last D, both formed exactly as
 *      compute_rnnt_tdt_greedy_step forms them (f32 partial sums per 32-column chunk, combined in float64 in slice order).  A
 *      waiting hypothesis reads nothing: a step evaluates the joint for active rows alone.
 *   2. Candidates: an active i offers (i, v, j) for every v < V, j < D with score
 *      s_i + (((double)logits_i[v] - lseT_i) + ((double)logits_i[V + j] - lseD_i)), the additions in that order; a waiting i offers
 *      the single (i, stay) with score s_i.  They are ranked by score descending, then i ascending, then stay before tokens, then v
 *      ascending, then j ascending, and the first `beam` are taken.  NaN and -inf candidates never are.
 *   3. Successors: (i, stay) gives (y_i, c_i).  (i, v, j) takes d = durations[j], and d = 1 if d == 0 (one symbol per frame, and
 *      a blank must move); its sequence is y_i when v == blank, else y_i + (v,); its cursor is t + d, which may pass T_b.  The
 *      sigma of the loss plays no part.
 *   4. Taken candidates with identical (sequence, cursor) merge: the first-ranked survives with the logaddexp of the scores, folded
 *      in rank order in float64.  The same sequence at different cursors does not merge: (i, v, 0) and (i, v, 1) under durations
 *      [0, 1, ...] do merge (both move one frame); a waiting (y, 5) and an active (y, 3) that takes the blank with d = 2 do too.
 *   5. The new beam is the merged list stably sorted by score, descending.  It may hold fewer than `beam` hypotheses.
 * If nothing is taken (every hypothesis active, none with a finite candidate) the beam is carried over with every cursor set to
 * t + 1.  Frames t >= T_b leave the beam as it is.
 * Consequences: beam = 1 is compute_rnnt_tdt_greedy_step with max_per_frame = 1 and no symbol budget (the independent argmaxes of
 * the two heads are the argmax of the sum, with the same tie order).  Restricting an active hypothesis to its `beam` best tokens,
 * and then to its `beam` best (v, j) pairs under (score, v, j), before the ranking changes nothing: a taken (i, v, j) is preceded
 * by (i, v', j) for every v' that beats v.
 *
 * compute_rnnt_tdt_beam_begin (once per decode) runs the greedy decoder's prepare path over all R columns, resets every beam and
 * stores the duration set.
 * compute_rnnt_tdt_beam_step (once per frame): pred_proj [minibatch * beam, joint_size]; parents / emitted i32 [minibatch * beam]
 * with the meaning they have in compute_rnnt_beam_step: slot k of utterance b continues row parents[b beam + k] and appended
 * emitted[...] (-1: nothing).  A stay gives its own parent and -1; empty slots and frozen utterances name their own row.  Optional
 * diagnostics (NULL: not written), written for the rows that were ACTIVE: topk_logits f32 / topk_symbols i32 [rows, beam], the token
 * head's best `beam` (logit descending, symbol ascending; -inf / -1 where fewer exist); dur_logits f32 [rows, D]; lse f32 [rows, 2]
 * = {token, duration}.  Every listed logit is bitwise that of compute_rnnt_joint_logits with alphabet_size = R for the hypothesis
 * alone, where compute_rnnt_beam_step gives that guarantee.
 * compute_rnnt_tdt_beam_results: hyps i32 [minibatch, beam, maxT] zero-padded, best first; hyp_lengths i32 and scores f32
 * [minibatch, beam] (empty slots: 0 and -inf); cursors i32 [minibatch, beam] or NULL (empty slots: -1); hyp_frames / hyp_durations
 * i32 [minibatch, beam, maxT], both given or both NULL and only with timed != 0: per token the frame that emitted it and the frames
 * it claims (the effective d, after d = 0 -> 1), -1 elsewhere.  A merged hypothesis keeps its first-ranked member's rows.
 *
 * 1 <= beam <= 16.  Shapes: every (joint_dtype, joint_size, R) that compute_rnnt_beam_step takes with alphabet_size = R; joint_dtype
 * carries no flag bits.  workspace: get_rnnt_tdt_beam_workspace_size bytes, 256-byte aligned, owned by one decode; it may hold
 * anything on entry.  Single stream, no global atomics, no memset, no entry point synchronises the host: two decodes of the same
 * input give the same bits, and an utterance's result does not depend on the batch around it.
 * RNNT_STATUS_INVALID_VALUE before anything is enqueued: every case compute_rnnt_beam_begin / _step / _results reject (a NULL
 * required pointer, a non-positive size, beam outside [1, 16], a joint_dtype other than 0 / 1, options.loc != RNNT_GPU,
 * options.batch_first == false, maxT or maxU < 1, a workspace that is NULL or not 256-byte aligned, a shape beyond the layout's
 * 2^31 limits); every durations / num_durations / alphabet_size / blank case compute_rnnt_tdt_greedy_begin rejects; hyp_frames /
 * hyp_durations with timed == 0; exactly one of the two NULL. */
RNNT_API rnntStatus_t get_rnnt_tdt_beam_workspace_size(int maxT, int minibatch, int beam, int joint_size, int alphabet_size,
                                                       int num_durations, int joint_dtype, int timed, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_tdt_beam_begin(const float *enc_proj, const int *frame_lengths, const float *W2, const float *b2,
                                                  int joint_size, int alphabet_size, const int *durations, int num_durations,
                                                  int minibatch, int beam, int joint_dtype, int timed, void *workspace,
                                                  rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_tdt_beam_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                                 int *topk_symbols, float *dur_logits, float *lse, int joint_size, int alphabet_size,
                                                 int num_durations, int minibatch, int beam, int joint_dtype, int timed,
                                                 void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_tdt_beam_results(int *hyps, int *hyp_lengths, float *scores, int *cursors, int *hyp_frames,
                                                    int *hyp_durations, int joint_size, int alphabet_size, int num_durations,
                                                    int minibatch, int beam, int joint_dtype, int timed, void *workspace,
                                                    rnntOptions options);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_TDT_BEAM_H */
