/* rnnt_beam_multi.h -- batched beam search with SEVERAL SYMBOLS PER FRAME (time-synchronous decoding on the standard lattice): an
 * extension of include/rnnt.h.
 *
 * include/rnnt.h and libwarprnnt.so, and every other extension header and library, stay as they are.  The four entry points declared
 * here are what libwarprnnt_multibeam.so exports, and all it exports; no other library holds anything of them.  The library links the
 * base library's kernel objects (the greedy decoder's prepare path and the per-hypothesis joint run unchanged) beside its own step,
 * select, begin and results kernels, and works on a workspace of its own.
 */
#ifndef RNNT_BEAM_MULTI_H
#define RNNT_BEAM_MULTI_H

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build-only extension (no upstream counterpart).  compute_rnnt_beam_* (include/rnnt.h) is the "modified" search: one symbol per
 * frame, then the next frame.  The loss of include/rnnt.h is on the STANDARD lattice, where a label edge stays on its frame, so a
 * model trained on it may emit any number of symbols in one frame.  This is the beam search for such a model: time-synchronous
 * decoding in the sense of Saon et al. 2020 (the "TSD" of ESPnet and NeMo), stated so that every step is a fixed amount of work and
 * no step reads the host.
 *
 * THE RULE.  Per utterance b: T_b = frame_lengths[b] clamped into [0, maxT]; blank = options.blank_label; K = beam (1 ... 16);
 * E = symbols_per_frame (1 ... 8); max_hyp_len >= 1.
 *
 * Two ordered lists of hypotheses (y, s), y a token sequence and s a float64 log score:
 *   A, the OPEN hypotheses: they sit at the current frame and may still emit;
 *   B, the CLOSED hypotheses: they have taken the frame's blank and wait at the next frame.
 * Each list holds at most K.  At the start A = [((), 0)] and B = [].
 *
 * One STEP is one ROUND for every utterance.  Step number k (counted from begin) is round r = k mod (E + 1) of frame
 * t = k div (E + 1).  Utterances with t >= T_b are left exactly as they are: every row gets parents = its own row and emitted = -1.
 * For t < T_b:
 *
 *   1. JOINT.  For every hypothesis i of A: logits_i = tanh(enc_proj[b, t] + pred_proj[row of i]) @ W2 + b2.  Every logit is bitwise
 *      that of compute_rnnt_joint_logits for the hypothesis alone.  lse_i is formed exactly as compute_rnnt_beam_step forms it: f32
 *      partial sums per 32-symbol chunk, combined in float64.  lp_i(v) = (double)logits_i[v] - lse_i.  B's rows are not evaluated.
 *
 *   2. CLOSINGS, in A's order: c_i = s_i + lp_i(blank).  A NaN or -inf c_i is skipped.  If B holds an entry with the sequence
 *      y_i, its score becomes logaddexp(score, c_i) in float64; the entry keeps its place in the insertion order, and it keeps its
 *      prediction-network state, which is the same for both because the sequence is the same.  Otherwise (y_i, c_i) is appended to
 *      B.  Then B is stably sorted by score, descending, and cut to its first K.  An open and a closed hypothesis with the same
 *      sequence are different lattice nodes and never merge.  Two open hypotheses of one round never share a sequence.
 *
 *   3. EXPANSIONS, in rounds r < E only.  Candidates are (i, v) with v != blank, len(y_i) < max_hyp_len, and score s_i + lp_i(v).
 *      They are ranked by score descending, then i ascending, then v ascending.  NaN and -inf candidates are never taken.  The
 *      first K become the new A, in that order, with sequences y_i + (v,).  In round r = E nothing expands.
 *
 *   4. FRAME TURN, at the end of round r = E: A := B (already sorted) and B := [].  If B is empty there, the utterance's beam is
 *      empty from then on: its results are length 0 and score -inf in every slot.
 *
 * The results after any whole number of frames are A, best first.
 *
 * ROWS AND PROTOCOL.  Rows are 2 K per utterance: A's slot k is row b 2K + k, B's slot k is row b 2K + K + k.  pred_proj is
 * [minibatch 2K, joint_size].  Every step writes parents and emitted (i32 [minibatch 2K]) for all 2 K rows:
 *   a new A slot gets the row of hypothesis i BEFORE THIS STEP and its v;
 *   a B slot gets the row that held that entry's state before this step (an A row for a fresh closing, a B row for an older entry)
 *     and -1;
 *   at the frame turn, the new A slot k gets the pre-step row of the entry ranked k, the B slots are emptied, and every emitted is -1;
 *   empty slots get their own row and -1.
 * All parents name pre-step rows.  compute_rnnt_prednet_step double-buffers by parity, so it serves this protocol unchanged with
 * rows = minibatch 2K.  A whole utterance takes T_b (E + 1) steps; the caller runs maxT (E + 1).
 *
 * compute_rnnt_multibeam_begin (once per decode) runs the greedy decoder's prepare path (the tables of enc_proj [minibatch, maxT,
 * joint_size], the W2 [joint_size, alphabet_size] operand image, b2 [alphabet_size]; all device f32, frame_lengths device i32
 * [minibatch]) and resets every utterance to A = [((), 0)], B = [].
 * compute_rnnt_multibeam_step: one step, as above.
 * compute_rnnt_multibeam_results: list A.  hyps i32 [minibatch, beam, max_hyp_len] zero-padded, best first; hyp_lengths i32 and
 * scores f32 [minibatch, beam] (empty slots: 0 and -inf).
 *
 * Shapes: every (joint_dtype, joint_size, alphabet_size) that compute_rnnt_beam_step takes; joint_dtype carries no flag bits.  The
 * same beam, symbols_per_frame, max_hyp_len, sizes and options.maxT in every call of one decode.  workspace:
 * get_rnnt_multibeam_workspace_size bytes, 256-byte aligned, owned by one decode; it may hold anything on entry.  Single stream, no
 * atomics, no memset, no entry point synchronises the host: two decodes of the same input give the same bits, and an utterance's
 * result does not depend on the batch around it.
 * RNNT_STATUS_INVALID_VALUE before anything is enqueued: every case compute_rnnt_beam_begin / _step / _results reject (a NULL
 * required pointer, a non-positive size, beam outside [1, 16], a joint_dtype other than 0 / 1, a blank outside the alphabet,
 * options.loc != RNNT_GPU, options.batch_first == false, maxT or maxU < 1, a workspace that is NULL or not 256-byte aligned, a shape
 * beyond the layout's 2^31 limits); symbols_per_frame outside [1, 8]; max_hyp_len < 1; minibatch * 2 * beam > 1024. */
RNNT_API rnntStatus_t get_rnnt_multibeam_workspace_size(int maxT, int minibatch, int beam, int symbols_per_frame, int max_hyp_len,
                                                        int joint_size, int alphabet_size, int joint_dtype, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_multibeam_begin(const float *enc_proj, const int *frame_lengths, const float *W2, const float *b2,
                                                   int joint_size, int alphabet_size, int minibatch, int beam, int symbols_per_frame,
                                                   int max_hyp_len, int joint_dtype, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_multibeam_step(const float *pred_proj, int *parents, int *emitted, int joint_size,
                                                  int alphabet_size, int minibatch, int beam, int symbols_per_frame, int max_hyp_len,
                                                  int joint_dtype, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_multibeam_results(int *hyps, int *hyp_lengths, float *scores, int joint_size, int alphabet_size,
                                                     int minibatch, int beam, int symbols_per_frame, int max_hyp_len, int joint_dtype,
                                                     void *workspace, rnntOptions options);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_BEAM_MULTI_H */
