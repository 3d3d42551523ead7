/* rnnt_modified_align.h -- forced alignment on the modified (one symbol per frame) lattice: an extension of include/rnnt.h.
 *
 * include/rnnt.h / libwarprnnt.so and include/rnnt_modified.h / libwarprnnt_mod.so stay as they are.  The four entry points
 * declared here are what libwarprnnt_modalign.so exports, and all it exports.  The extension library is self-contained: its own
 * kernels, its own workspace, nothing shared with the other libraries but the types of rnnt.h.
 */
#ifndef RNNT_MODIFIED_ALIGN_H
#define RNNT_MODIFIED_ALIGN_H

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build-only extension (no upstream counterpart): FORCED ALIGNMENT ON THE MODIFIED LATTICE -- the maximum-probability path among
 * the paths compute_rnnt_loss_modified (include/rnnt_modified.h) sums over: every frame emits exactly ONE of {blank, next label}.
 * It is the max-plus twin of that loss and the aligner that goes with a model trained on it; compute_rnnt_align (include/rnnt.h)
 * keeps the standard lattice, where several labels may share a frame.
 *
 * Conventions of compute_rnnt_align: acts f32 [minibatch, maxT, maxU, alphabet_size] RAW LOGITS, T = input_lengths[b],
 * L = label_lengths[b], flat_labels [minibatch, maxU-1], blank = options.blank_label,
 *   lpb[t,u] = log_softmax(acts[b,t,u,:])[blank],   lpl[t,u] = log_softmax(acts[b,t,u,:])[label_b[u]]   (u < L).
 * Nodes (t,u), 0 <= t <= T, 0 <= u <= L; every edge advances the frame:
 *   v(0,0) = 0,  v(0,u>0) = -inf
 *   v(t,u) = max( v(t-1,u) + lpb[t-1,u] ,  v(t-1,u-1) + lpl[t-1,u-1] )        (second term for u >= 1)
 *   score  = v(T,L)                                                            (no final blank)
 * Tie rule (part of the contract): the label arrival, from (t-1,u-1), is taken only if it is STRICTLY greater; on an exact tie
 * the blank arrival, from (t-1,u), wins.  A node with one reachable predecessor takes that one.
 * Back-trace: it starts at (T,L) and takes one step per frame; a label arrival into (t,u) sets
 *   token_frames[u-1] = t-1,   token_logp[u-1] = lpl[t-1,u-1].
 * Outputs (the shapes and padding of compute_rnnt_align):
 *   token_frames  device i32 [minibatch, maxU-1]  the frame that emits label u; -1 for u >= L.  STRICTLY increasing in u.
 *   token_logp    device f32 [minibatch, maxU-1]  the label's log-probability there; 0 for u >= L
 *   scores        device f32 [minibatch]          the best path's log-probability (natural log); never above -cost of
 *                                                 compute_rnnt_loss_modified on the same inputs
 * L = 0 is valid: the path is all blanks.  L > T has no path; that is legitimate data, not an error: the score is -inf, every
 * frame -1, every token_logp 0, never a NaN.  Out-of-range lengths (T < 1, T > maxT, L < 0, L > maxU-1) are device data: they
 * are clamped into the tensor and THAT utterance alone comes back with a NaN score, -1 frames and 0 confidences.  Labels outside
 * [0, alphabet_size) are clamped into it.
 * Arithmetic: the normaliser of every cell in float32 from the float32 logits (running max / sum of exponentials) in an order
 * fixed by alphabet_size alone; v is carried in float64.  An utterance's three outputs are BITWISE independent of the rest of the
 * batch, of minibatch and of how the frames were cut into slabs.  A path passes through cell (t,u), t < T, only inside the band
 * u <= t, L - u <= T - t: cells outside the band, and cells outside an utterance's lattice, are read neither from acts nor from
 * the workspace.
 *
 *   get_rnnt_modified_align_workspace_size  bytes for (maxT, maxU, minibatch): two f32 per lattice cell, row-major [t][u] on a row
 *                                  stride of maxU rounded up to the sweep's width (64 x columns per lane; 1024 x columns per
 *                                  thread above 1024 columns), and one decision BIT per node.  Never depends on alphabet_size.
 *                                  The workspace may hold anything on entry.
 *   compute_rnnt_modified_align_cells  acts_slab f32 [minibatch, slab_frames, maxU, alphabet_size] = the logits of frames
 *                                  frame_offset ... frame_offset + slab_frames - 1 of every utterance: writes lpb / lpl of their
 *                                  in-band cells into the workspace.
 *   compute_rnnt_modified_align_path   the sweep and the back-trace, in one launch, on what a sequence of _cells calls covering
 *                                  frames 0 ... maxT-1 (in any order, any slab sizes) has left in the workspace.
 *   compute_rnnt_modified_align    = _cells on the whole tensor (slab_frames = maxT, frame_offset 0) followed by _path.
 * Domain: that of compute_rnnt_align -- maxU <= 8192, minibatch * maxT * maxU < 2^31, any alphabet_size >= 2,
 * 0 <= blank_label < alphabet_size, options.loc == RNNT_GPU, batch_first; 1 <= slab_frames, 0 <= frame_offset,
 * frame_offset + slab_frames <= maxT.  Pointers: none may be NULL; workspace 256-byte aligned, every other 4-byte aligned
 * (acts_slab 16-byte aligned with alphabet_size a multiple of 4 takes the wide loads; results do not depend on it).  Anything
 * else: RNNT_STATUS_INVALID_VALUE before anything is enqueued.  Everything is enqueued on options.stream; no entry point
 * synchronises the host. */
RNNT_API rnntStatus_t get_rnnt_modified_align_workspace_size(int maxT, int maxU, int minibatch, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_modified_align_cells(const float *acts_slab, int slab_frames, int frame_offset,
                                                        const int *flat_labels, const int *label_lengths,
                                                        const int *input_lengths, int alphabet_size, int minibatch,
                                                        void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_modified_align_path(int *token_frames, float *token_logp, float *scores,
                                                       const int *label_lengths, const int *input_lengths, int minibatch,
                                                       void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_modified_align(const float *acts, const int *flat_labels, const int *label_lengths,
                                                  const int *input_lengths, int alphabet_size, int minibatch,
                                                  int *token_frames, float *token_logp, float *scores, void *workspace,
                                                  rnntOptions options);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_MODIFIED_ALIGN_H */
