/* rnnt_tdt_beam_stream.h -- chunked streaming beam search of a token-and-duration (TDT) transducer with per-stream beam slots: an
 * extension of include/rnnt.h.
 *
 * include/rnnt.h, include/rnnt_tdt_beam.h, include/rnnt_tdt_stream.h and their libraries stay as they are.  The five entry points
 * declared here are what libwarprnnt_tdtbeamstream.so exports, and all it exports; no other library holds anything of them.  The
 * library links the base library's kernel objects (the greedy stream's chunk projection, the W2 image and the per-hypothesis joint
 * run unchanged) beside its own begin, feed, step, select and results kernels; its step and select kernels are compiled from the
 * text of libwarprnnt_tdtbeam.so's.  It works on a workspace of its own.
 */
#ifndef RNNT_TDT_BEAM_STREAM_H
#define RNNT_TDT_BEAM_STREAM_H

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build-only extension (no upstream counterpart): BEAM SEARCH of the token-and-duration transducer OVER A STREAM OF CHUNKS per
 * slot -- compute_rnnt_beam_stream_begin / _feed / _step / _results (include/rnnt.h) with the rule of compute_rnnt_tdt_beam_step
 * (include/rnnt_tdt_beam.h).  `slots` streams are decoded side by side; each slot holds one stream at a time, keeps its beam from
 * one feed to the next, and its encoder frames arrive chunk by chunk.  The caller steps the prediction network.
 *
 * Arguments and limits: those of compute_rnnt_beam_stream_*.  S = slots, K = beam, N = max_hyp_len (the tokens a hypothesis may
 * hold); 1 <= K <= 16, 1 <= S, S K <= 1024, 1 <= N, 2 S K N < 2^31 (timed: 6 S K N), 1 <= enc_width <= 4096; options.maxT =
 * max_chunk_frames, the same options in every call.  enc [slots, enc_frames, enc_width] device f32 (NULL allowed when enc_frames is
 * 0), enc_frames in [0, options.maxT], chunk_frames [slots], reset / final_chunk [slots] or NULL.  V = alphabet_size tokens (blank
 * included), D = num_durations, R = V + D; W2 [joint_size, R] and b2 [R] with the V token columns first; the duration set, the
 * alphabet and the blank obey compute_rnnt_tdt_beam_begin's rules; durations is a HOST int [D], read during begin only and handed on
 * as kernel arguments.  timed: 0 / non-zero, the same in every call: non-zero keeps per token its frame and duration.
 *
 * Workspace: get_rnnt_tdt_beam_stream_workspace_size bytes, 256-byte aligned, owned by the decoder from begin on; it may hold
 * anything on entry.  It is the TDT beam workspace at (max_chunk_frames, S, K) with token and pair rows of stride N instead of
 * maxT, then W1 [enc_width, joint_size] and b1 as the beam stream keeps them, then one int per slot: the slot's FRAME BASE, the
 * frames of the chunks it has left behind since its reset.  The workspace owns the frame base: the caller carries no state.
 *
 * A hypothesis is (y, c, s) as in include/rnnt_tdt_beam.h.  Inside the library its cursor c counts from the first frame of the chunk
 * its slot holds, so what a duration jump reached beyond that chunk is carried across feeds per hypothesis; every cursor and frame
 * that leaves the library counts from the slot's reset (frame base + chunk-local value).
 *
 * compute_rnnt_tdt_beam_stream_begin (once) packs W1, b1, the W2 image over all R columns and the duration set (the caller may
 * then free them), and leaves every slot FINISHED with an EMPTY beam (no hypothesis at all).
 *
 * compute_rnnt_tdt_beam_stream_feed projects the chunk through W1 + b1 with the greedy stream's projection (one f32 FMA chain per
 * output: a frame's enc_proj is bitwise independent of the chunking, the slot and S), builds the e^{2x} tables and range flags of
 * those frames, and moves every slot on.  Per slot s, in this order (Tb_old: the frames of the chunk the slot held):
 *   1. reset[s] != 0:        the beam becomes [((), 0, 0)], the step count 0, base = 0, and the slot is not finished.
 *   2. otherwise, a slot that is not finished: base += Tb_old, and every occupied hypothesis gets cursor = max(cursor - Tb_old,
 *      0).  The cursors of one beam shift together, so rule 4 (merging on (sequence, cursor)) is unaffected.
 *   3. a finished slot stays frozen, its beam readable, until a reset.
 *   4. a live slot gets frame counter 0 over clamp(chunk_frames[s], 0, enc_frames) frames; final_chunk[s] != 0 finishes it after
 *      this chunk, and a carry beyond a final chunk is dropped.
 * A hypothesis whose carry exceeds the new chunk waits through all of it, offering its `stay` each frame, and carries on by the
 * same formula.  A feed is legal once the previous chunk's steps have run; the clamp to 0 exists only so that no out-of-range
 * frame can be addressed otherwise.
 *
 * compute_rnnt_tdt_beam_stream_step: one frame of every slot that has one left in its chunk, by rules 1 - 5 of
 * include/rnnt_tdt_beam.h with minibatch = slots, with the same outputs and diagnostics (pred_proj [S K, joint_size]; parents /
 * emitted i32 [S K]; topk_logits / topk_symbols [S K, K], dur_logits [S K, D], lse [S K, 2] or NULL).  Slots without a frame left
 * are frozen: parents = own row, emitted = -1.  The arithmetic is bitwise compute_rnnt_tdt_beam_step's: f32 partials per
 * 32-column chunk, their float64 combination in slice order, float64 scores.  One rule is added, the analogue of the beam stream's:
 * an ACTIVE hypothesis that already holds N tokens offers only its D candidates (i, blank, j), whatever rank the blank has among
 * its token logits; its other candidates are never taken, exactly like -inf candidates (topk_logits / topk_symbols still show its
 * plain top-`beam`).  The rule cannot fire in compute_rnnt_tdt_beam_step.
 *
 * compute_rnnt_tdt_beam_stream_results: the current beams, best first, in the form of compute_rnnt_tdt_beam_results with rows of
 * stride N: hyps i32 [S, K, N] zero-padded; hyp_lengths i32 and scores f32 [S, K]; cursors i32 [S, K] or NULL, counted from the
 * slot's reset; stable_lengths i32 [S] or NULL: the length of the longest common token prefix of all occupied hypotheses of the
 * slot; hyp_frames / hyp_durations i32 [S, K, N] (both given or both NULL, timed only; -1 padded): per token the frame since the
 * slot's reset that emitted it and the frames it claims; timed_stable_lengths i32 [S] or NULL (timed only): the prefix on which the
 * occupied hypotheses agree in token, frame and duration, never more than stable_lengths.  An empty or never-started slot: lengths
 * 0, scores -inf, cursors -1, both stable lengths 0.  Callable between any two calls of the stream; it changes nothing.
 *
 * The loop, per chunk: feed; then max over s of chunk_frames[s] times {compute_rnnt_tdt_beam_stream_step;
 * compute_rnnt_prednet_step(emitted, parents)}.  The number of steps is host data: nothing is polled.  The prediction network is
 * stepped after the LAST frame of a feed too.  A new stream in slot s resets its K prediction-network rows.
 *
 * EQUIVALENCE.  A stream fed through any chunking -- 0-frame feeds, 1-frame chunks and chunks shorter than a pending carry
 * included --, in any slot, beside any other traffic, ends with bitwise the n-best ids, lengths, f32 scores, cursors, frames,
 * durations and both stable lengths of the same stream fed in one chunk to a 1-slot decoder.
 *
 * Single stream, no global atomics, no memset.  No entry point synchronises the host.
 * RNNT_STATUS_INVALID_VALUE before anything is enqueued: every case compute_rnnt_beam_stream_begin / _feed / _step / _results
 * reject at alphabet_size = R (a NULL required pointer, a misaligned pointer -- workspace: 256 bytes, every other: 4 --, a shape
 * outside the limits above, enc_frames outside [0, options.maxT], a joint_dtype other than 0 / 1, options.loc != RNNT_GPU,
 * options.batch_first == false, maxT or maxU < 1); every durations / num_durations / alphabet_size / blank case
 * compute_rnnt_tdt_beam_begin rejects; hyp_frames / hyp_durations / timed_stable_lengths with timed == 0; exactly one of hyp_frames
 * / hyp_durations NULL.  get_rnnt_tdt_beam_stream_workspace_size returns it for a NULL size_bytes and for the same shape limits. */
RNNT_API rnntStatus_t get_rnnt_tdt_beam_stream_workspace_size(int max_chunk_frames, int slots, int beam, int max_hyp_len,
                                                              int enc_width, int joint_size, int alphabet_size, int num_durations,
                                                              int joint_dtype, int timed, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_tdt_beam_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2,
                                                         int enc_width, int joint_size, int alphabet_size, const int *durations,
                                                         int num_durations, int slots, int beam, int max_hyp_len, int joint_dtype,
                                                         int timed, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_tdt_beam_stream_feed(const float *enc, int enc_frames, const int *chunk_frames, const int *reset,
                                                        const int *final_chunk, int enc_width, int joint_size, int alphabet_size,
                                                        int num_durations, int slots, int beam, int max_hyp_len, int joint_dtype,
                                                        int timed, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_tdt_beam_stream_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                                        int *topk_symbols, float *dur_logits, float *lse, int joint_size,
                                                        int alphabet_size, int num_durations, int slots, int beam, int max_hyp_len,
                                                        int joint_dtype, int timed, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_tdt_beam_stream_results(int *hyps, int *hyp_lengths, float *scores, int *cursors,
                                                           int *stable_lengths, int *hyp_frames, int *hyp_durations,
                                                           int *timed_stable_lengths, int joint_size, int alphabet_size,
                                                           int num_durations, int slots, int beam, int max_hyp_len, int joint_dtype,
                                                           int timed, void *workspace, rnntOptions options);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_TDT_BEAM_STREAM_H */
