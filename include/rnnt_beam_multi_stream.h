/* rnnt_beam_multi_stream.h -- chunked streaming beam search with SEVERAL SYMBOLS PER FRAME (time-synchronous decoding on the
 * standard lattice) with per-stream beam slots: an extension of include/rnnt.h.
 *
 * include/rnnt.h, include/rnnt_beam_multi.h and their libraries stay as they are.  The five entry points declared here are what
 * libwarprnnt_multibeamstream.so exports, and all it exports; no other library holds anything of them.  The library links the base
 * library's kernel objects (the greedy stream's chunk projection, the W2 image and the per-hypothesis joint run unchanged) beside its
 * own begin, feed, step, select and results kernels; its step and select kernels are compiled from the text of
 * libwarprnnt_multibeam.so's.  It works on a workspace of its own.
 */
#ifndef RNNT_BEAM_MULTI_STREAM_H
#define RNNT_BEAM_MULTI_STREAM_H

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build-only extension (no upstream counterpart): the search of include/rnnt_beam_multi.h OVER A STREAM OF CHUNKS per slot -- the
 * protocol of compute_rnnt_beam_stream_begin / _feed / _step / _results (include/rnnt.h) with rules 1 - 4 of
 * include/rnnt_beam_multi.h.  `slots` streams are decoded side by side; each slot holds one stream at a time, keeps its lists from
 * one feed to the next, and its encoder frames arrive chunk by chunk.  The caller steps the prediction network.
 *
 * Arguments and limits.  S = slots, K = beam (1 ... 16), E = symbols_per_frame (1 ... 8), N = max_hyp_len >= 1 (the tokens a
 * hypothesis may hold); S 2K <= 1024 (the prediction network's rows); 4 S K N < 2^31, and with `timed` 8 S K N < 2^31;
 * 1 <= enc_width <= 4096; options.maxT = max_chunk_frames, the same options in every call.  Every (joint_dtype, joint_size,
 * alphabet_size) that compute_rnnt_multibeam_step takes; joint_dtype carries no flag bits.  enc [slots, enc_frames, enc_width]
 * device f32 (NULL allowed when enc_frames is 0), enc_frames in [0, options.maxT], chunk_frames [slots] device i32, reset /
 * final_chunk [slots] device i32 or NULL.  timed: 0 / non-zero, the same in every call: non-zero keeps per token its emission frame.
 *
 * Rows are 2 K per slot: slot s's open list A has its entry k on row s 2K + k, its closed list B on row s 2K + K + k.  pred_proj
 * [S 2K, joint_size], parents and emitted (i32 [S 2K]) cover all rows and mean what they mean in include/rnnt_beam_multi.h; all
 * parents name pre-step rows, so compute_rnnt_prednet_step serves with rows = S 2K.
 *
 * Workspace: get_rnnt_multibeam_stream_workspace_size bytes, 256-byte aligned, owned by the decoder from begin on; it may hold
 * anything on entry.  It is the workspace of include/rnnt_beam_multi.h at (max_chunk_frames, S, K), then one int per slot, the
 * slot's FRAME BASE (the frames of the chunks it has left behind since its reset), then with `timed` a second double-buffered int
 * row per hypothesis (the frames), then W1 [enc_width, joint_size] and b1 as the beam stream keeps them.  The workspace owns the
 * frame base: the caller carries no state.
 *
 * compute_rnnt_multibeam_stream_begin (once): packs W1, b1 and the W2 operand image; leaves every slot FINISHED with an EMPTY
 * beam, as compute_rnnt_beam_stream_begin does.
 *
 * compute_rnnt_multibeam_stream_feed: projects the chunk through W1 + b1 with the greedy stream's projection (one f32 FMA chain
 * per output, so a frame's enc_proj is bitwise independent of the chunking, the slot and S), builds the tables of the chunk's frames,
 * and moves every slot on:
 *   reset[s] != 0:  A = [((), 0)], B = [], step count 0, frame base 0, not finished;
 *   a live slot:    frame base += the frames of the chunk it held; its frame counter is 0 over clamp(chunk_frames[s], 0,
 *                   enc_frames) frames; round 0, B = []; A and the step count are kept;
 *   a finished one: stays frozen and readable until a reset.
 * final_chunk[s] != 0 finishes the slot after this chunk.  A feed is legal once all max_s chunk_frames[s] (E + 1) steps of the
 * feed before it have run.  A feed that comes earlier drops the unfinished rounds (B is emptied, the round is 0): that rule is
 * there so that no state can leave its range, and is no part of the equivalence below.
 *
 * compute_rnnt_multibeam_stream_step: one ROUND of every slot that has a frame left in its chunk: step k since the feed is round
 * k mod (E + 1) of chunk frame k div (E + 1), by rules 1 - 4 of include/rnnt_beam_multi.h with minibatch = slots; the arithmetic
 * is bitwise that of compute_rnnt_multibeam_step.  Slots without a frame left are frozen (parents = own row, emitted = -1).  The
 * capacity rule is rule 3: a hypothesis of N tokens offers no expansion, and goes on closing on blanks.  The prediction network is
 * stepped after the last step of a feed too.
 *
 * compute_rnnt_multibeam_stream_results: list A, best first.  hyps i32 [S, K, N] zero-padded, hyp_lengths i32 [S, K], scores
 * f32 [S, K].  stable_lengths i32 [S] or NULL: the longest common token prefix of the occupied hypotheses of A.  The stability
 * claim holds AT FRAME BOUNDARIES ONLY (after a whole number of frames, e.g. once all steps of a feed have run): there B is empty and
 * every later hypothesis extends one of A, so that prefix can no longer change; between the rounds of a frame A holds this frame's
 * expansions alone and the prefix means nothing final.  With `timed`: hyp_frames i32 [S, K, N] (-1 padded) or NULL, per token the
 * frame since the slot's reset (frame base + chunk frame) whose joint evaluation appended it, under the definition of emission
 * frames in include/rnnt.h; timed_stable_lengths i32 [S] or NULL, the prefix on which the hypotheses agree in token and frame,
 * never more than stable_lengths.  Frames under a merge: when a closing is added into an entry B already holds, the entry keeps
 * ITS OWN frame row, as it keeps its prediction-network state; the score is the logaddexp.  Frames describe one path while the
 * score may sum several.  An empty or never-started slot gives lengths 0, scores -inf and both stable lengths 0.  Callable between
 * any two calls; it changes nothing.
 *
 * EQUIVALENCE.  A stream fed through any chunking (0-frame feeds, 1-frame chunks and an empty final feed included), in any slot,
 * beside any other traffic, ends bitwise equal -- n-best ids, lengths, f32 scores, stable_lengths, hyp_frames,
 * timed_stable_lengths -- to the same stream fed in one chunk to a 1-slot decoder.  Ids, lengths and f32 scores are also bitwise
 * those of compute_rnnt_multibeam_begin / _step / _results run offline on the same enc_proj at max_hyp_len = N.  The timed and the
 * untimed stream agree bitwise in everything both report.
 *
 * Single stream, no global atomics, no memset, no entry point synchronises the host.
 * RNNT_STATUS_INVALID_VALUE before anything is enqueued: every case compute_rnnt_beam_stream_* and compute_rnnt_multibeam_*
 * reject (a NULL required pointer, a pointer that is not 4-byte aligned, a non-positive size, beam outside [1, 16], a joint_dtype
 * other than 0 / 1, a blank outside the alphabet, options.loc != RNNT_GPU, options.batch_first == false, maxT or maxU < 1, a
 * workspace that is NULL or not 256-byte aligned, max_hyp_len < 1, enc_width outside [1, 4096]); symbols_per_frame outside
 * [1, 8]; S 2K > 1024; the 2^31 limits above; hyp_frames or timed_stable_lengths given with timed == 0; enc_frames outside
 * [0, options.maxT]. */
RNNT_API rnntStatus_t get_rnnt_multibeam_stream_workspace_size(int max_chunk_frames, int slots, int beam, int symbols_per_frame,
                                                               int max_hyp_len, int enc_width, int joint_size, int alphabet_size,
                                                               int joint_dtype, int timed, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_multibeam_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2,
                                                          int enc_width, int joint_size, int alphabet_size, int slots, int beam,
                                                          int symbols_per_frame, int max_hyp_len, int joint_dtype, int timed,
                                                          void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_multibeam_stream_feed(const float *enc, int enc_frames, const int *chunk_frames, const int *reset,
                                                         const int *final_chunk, int enc_width, int joint_size, int alphabet_size,
                                                         int slots, int beam, int symbols_per_frame, int max_hyp_len, int joint_dtype,
                                                         int timed, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_multibeam_stream_step(const float *pred_proj, int *parents, int *emitted, int joint_size,
                                                         int alphabet_size, int slots, int beam, int symbols_per_frame,
                                                         int max_hyp_len, int joint_dtype, int timed, void *workspace,
                                                         rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_multibeam_stream_results(int *hyps, int *hyp_lengths, float *scores, int *stable_lengths,
                                                            int *hyp_frames, int *timed_stable_lengths, int joint_size,
                                                            int alphabet_size, int slots, int beam, int symbols_per_frame,
                                                            int max_hyp_len, int joint_dtype, int timed, void *workspace,
                                                            rnntOptions options);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_BEAM_MULTI_STREAM_H */
