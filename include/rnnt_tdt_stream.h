/* rnnt_tdt_stream.h -- chunked streaming greedy decoding of a token-and-duration (TDT) transducer with per-stream state slots: an
 * extension of include/rnnt.h.
 *
 * include/rnnt.h, include/rnnt_tdt.h and include/rnnt_tdt_greedy.h and their libraries stay as they are.  The four entry points
 * declared here are what libwarprnnt_tdtstream.so exports, and all it exports; no other library holds anything of them.  The
 * library links the base library's kernel objects (the greedy stream's chunk projection and the per-hypothesis joint run
 * unchanged) and the batched TDT greedy decoder's object (its step kernel runs unchanged) beside its own feed and update kernels,
 * and works on a workspace of its own.
 */
#ifndef RNNT_TDT_STREAM_H
#define RNNT_TDT_STREAM_H

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build-only extension (no upstream counterpart): GREEDY DECODING of the token-and-duration transducer OVER A STREAM OF CHUNKS per
 * slot -- compute_rnnt_greedy_stream_begin / _feed (include/rnnt.h) with the step rule of compute_rnnt_tdt_greedy_step
 * (include/rnnt_tdt_greedy.h).  `slots` streams are decoded side by side; each slot holds one stream at a time, and its encoder
 * frames arrive chunk by chunk.  The caller steps the prediction network.
 *
 * Arguments.  enc [slots, enc_frames, enc_width] device f32, enc_frames in [0, options.maxT], chunk_frames [slots], reset / final_chunk
 * / max_symbols [slots] or NULL, options.maxT = max_chunk_frames and 1 <= slots <= 1024, 1 <= enc_width <= 4096: those of
 * compute_rnnt_greedy_stream_begin / _feed.  V = alphabet_size tokens (blank included), D = num_durations, R = V + D; W2
 * [joint_size, R] and b2 [R] with the V token columns first; durations HOST int [D], read during begin only and handed on as kernel
 * arguments; hyps, hyp_frames / hyp_logp (both given or both NULL), hyp_lengths, scores, emitted, all_done and logit_stats
 * [slots, 4]: those of compute_rnnt_tdt_greedy_begin / _step.  The duration set obeys the rule of include/rnnt_tdt.h.
 *
 * Workspace: get_rnnt_tdt_greedy_stream_workspace_size bytes, 256-byte aligned, owned by the decoder from begin on; it may hold
 * anything on entry.  It is the TDT greedy workspace at (max_chunk_frames, slots), then W1 [enc_width, joint_size] and b1 as the
 * greedy stream keeps them, then one int per slot: the slot's FRAME BASE, the frames of the chunks it has left behind since its
 * reset.  The frame base is owned by the workspace: unlike compute_rnnt_greedy_stream_feed_timed, the caller carries no state.
 *
 * compute_rnnt_tdt_greedy_stream_begin (once) builds the W2 operand image over all R columns, copies W1 / b1, stores the duration set
 * and leaves every slot FINISHED: a slot decodes nothing until a feed resets it.
 *
 * compute_rnnt_tdt_greedy_stream_feed hands every slot its chunk.  Per slot s, in this order (t, n, nf: frame cursor, symbols emitted,
 * symbols emitted on the current frame; Tb: frames of the chunk the slot holds; _old: before this feed):
 *   1. reset[s] != 0:  n = 0, score = 0, fin = 0, base = 0, skip = 0; budget = max(max_symbols[s], 0), unlimited when max_symbols is
 *      NULL; cap = max_per_frame.
 *   2. otherwise:      base += Tb_old; skip = max(t_old - Tb_old, 0) -- what the slot's last duration jump reached beyond the chunk it
 *      held (at most durations[D-1] - 1 <= 7 frames; 0 for a slot that was finished).
 *   3. fin or n >= budget: the slot is finished (fin = 1, Tb = 0, done) until a reset.
 *   4. otherwise:      Tb = clamp(chunk_frames[s], 0, enc_frames); t = skip; nf = 0; fin = 1 if final_chunk[s] != 0 (it takes effect
 *      after this chunk: a carry beyond a final chunk is dropped); done = (t >= Tb).
 * So a slot whose carry exceeds the new chunk does nothing in this feed and carries t - Tb on, by the same formula, at the next.
 * The chunk goes through W1 + b1 with the greedy stream's own projection: every enc_proj value is one FMA chain over the encoder
 * width in order, then + b1, so a frame's enc_proj is bitwise independent of the chunking, the slot and `slots`.  Feed writes
 * hyp_lengths, scores and all_done (0: some slot has frames to decode, 1: none).  A feed is legal once the step loop has reported
 * all_done == 1; after a pause (all_done == 2) the caller grows hyps / hyp_frames / hyp_logp and goes on stepping, as for the
 * batched decoder.
 *
 * compute_rnnt_tdt_greedy_stream_step is compute_rnnt_tdt_greedy_step on the slots: the same two argmaxes (lowest index on ties), the
 * same float64 log-softmaxes, the same forcing of d = 0 to 1 after a blank or at the cap, t += d (which may pass Tb), done when
 * t >= Tb or n >= budget, the paused state 2, a head without a finite logit counted as blank / d = 1 with a NaN score -- and the step
 * kernel itself is that decoder's, so the numerics are those of include/rnnt_tdt_greedy.h.  The one difference:
 * hyp_frames[s, n] = base + t, the frame since the slot's reset.
 *
 * EQUIVALENCE.  A stream fed through any chunking -- 0-frame feeds and 1-frame chunks included --, in any slot, beside any other
 * traffic, ends with bitwise the ids, frames, log-probabilities, length and score of the same stream fed in one chunk to a 1-slot
 * decoder.
 *
 * Single stream, no atomics, no memset.  No entry point synchronises the host.
 * RNNT_STATUS_INVALID_VALUE before anything is enqueued: every case compute_rnnt_greedy_stream_begin / _feed reject (a NULL required
 * pointer -- enc may be NULL when enc_frames is 0 --, enc_frames outside [0, options.maxT], slots outside [1, 1024], enc_width outside
 * [1, 4096], a workspace that is NULL or not 256-byte aligned, and the cases of compute_rnnt_greedy_begin: a non-positive size, a
 * joint_dtype other than 0 / 1, options.loc != RNNT_GPU, options.batch_first == false, maxT or maxU < 1, slots * maxT * joint_size >=
 * 2^31); every case compute_rnnt_tdt_greedy_begin / _step reject (a durations array that breaks the rule, or NULL; num_durations
 * outside [1, 8]; alphabet_size < 2; the blank outside [0, alphabet_size); max_hyp_len < 1 or max_hyp_len * slots >= 2^31; exactly
 * one of hyp_frames / hyp_logp NULL; hyps, hyp_frames or hyp_logp not 4-byte aligned; a (joint_dtype, joint_size, R) the greedy decoder
 * does not take); max_per_frame < 1 in feed.  get_rnnt_tdt_greedy_stream_workspace_size returns it for a NULL size_bytes and for the
 * same shape limits. */
RNNT_API rnntStatus_t get_rnnt_tdt_greedy_stream_workspace_size(int max_chunk_frames, int slots, int enc_width, int joint_size,
                                                                int alphabet_size, int num_durations, int joint_dtype,
                                                                size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_tdt_greedy_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2,
                                                           int enc_width, int joint_size, int alphabet_size, const int *durations,
                                                           int num_durations, int slots, int joint_dtype, void *workspace,
                                                           rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_tdt_greedy_stream_feed(const float *enc, int enc_frames, const int *chunk_frames, const int *reset,
                                                          const int *final_chunk, const int *max_symbols, int max_per_frame,
                                                          int *hyp_lengths, float *scores, int *all_done, int enc_width,
                                                          int joint_size, int alphabet_size, int num_durations, int slots,
                                                          int joint_dtype, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_tdt_greedy_stream_step(const float *pred_proj, int *hyps, int *hyp_frames, float *hyp_logp,
                                                          int max_hyp_len, int *hyp_lengths, float *scores, int *emitted,
                                                          int *all_done, float *logit_stats, int joint_size, int alphabet_size,
                                                          int num_durations, int slots, int joint_dtype, void *workspace,
                                                          rnntOptions options);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_TDT_STREAM_H */
