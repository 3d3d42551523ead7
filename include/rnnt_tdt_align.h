/* rnnt_tdt_align.h -- forced alignment on the token-and-duration (TDT) lattice: an extension of include/rnnt.h.
 *
 * include/rnnt.h / libwarprnnt.so and include/rnnt_tdt.h / libwarprnnt_tdt.so stay as they are.  The four entry points declared
 * here are what libwarprnnt_tdtalign.so exports, and all it exports.  The extension library is self-contained: its own kernels,
 * its own workspace, nothing shared with the other libraries but the types of rnnt.h.
 */
#ifndef RNNT_TDT_ALIGN_H
#define RNNT_TDT_ALIGN_H

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build-only extension (no upstream counterpart): FORCED ALIGNMENT ON THE TDT LATTICE -- the maximum-probability path among the
 * paths compute_rnnt_loss_tdt (include/rnnt_tdt.h) sums over, and per label the frame that emits it and the number of frames it
 * claims.  It is the max-plus twin of that loss and the aligner that goes with a model trained on it; compute_rnnt_align
 * (include/rnnt.h) and compute_rnnt_modified_align keep their own lattices and know nothing of duration logits.
 *
 * Conventions of compute_rnnt_loss_tdt: acts f32 [minibatch, maxT, maxU, V + D] RAW LOGITS, V = alphabet_size token logits (blank
 * included), then D = num_durations duration logits; T = input_lengths[b], L = label_lengths[b], flat_labels [minibatch, maxU-1]
 * = y_0 ... y_{L-1}, blank = options.blank_label, maxT / maxU = options.maxT / options.maxU,
 *   lp(t,u,v) = log_softmax(acts[b,t,u,:V])[v],   ld(t,u,i) = log_softmax(acts[b,t,u,V:])[i]     -- two separate log-softmaxes
 *   durations   HOST int [D], read during the call: strictly increasing, durations[0] in {0, 1}, some d > 0 present,
 *               1 <= D <= 8, durations[D-1] <= 8 (the rule of include/rnnt_tdt.h);  sigma >= 0, finite (tokens only).
 * Lattice (that of include/rnnt_tdt.h).  Nodes (t,u), 0 <= t < T, 0 <= u <= L, and the terminal (T, L).  From (t,u), for each i with
 * d = durations[i]:
 *   blank edge to (t+d, u),    wb_i = ((x[blank] - lseV) - sigma) + (x[V+i] - lseD);  iff d > 0 and (t+d < T, or t+d == T and u == L)
 *   label edge to (t+d, u+1),  wl_i = ((x[y_u]   - lseV) - sigma) + (x[V+i] - lseD);  iff u < L and t+d < T
 * in float32, every operation rounded once, lseV / lseD the float32 normalisers (running max / sum of exponentials, in an order
 * fixed by V + D alone).
 *   v(0,0) = 0;  v(node) = max over incoming edges of v(source) + (double) w, carried in float64;  scores[b] = v(T, L)
 * Tie rule (part of the contract): the incoming candidates of a node are scanned in increasing i, for each i the blank arrival (from
 * (t-d_i, u)) before the label arrival (from (t-d_i, u-1)) -- the order of the loss's sum -- and a candidate replaces the incumbent
 * only if it is STRICTLY greater.  A node keeps one decision code: 2 i + (1 for a label arrival).
 * Back-trace: from (T, L); a label arrival into (t,u) over duration i sets
 *   token_frames[u-1] = t - d_i,  token_durations[u-1] = d_i,  token_logp[u-1] = lp(t-d_i, u-1, y_{u-1}) + ld(t-d_i, u-1, i)
 * -- the log-probability of the token and of its duration WITHOUT sigma, what the TDT decoders report per token.  It is recovered
 * from the stored weight as wl_i + sigma (float32): bit for bit lp + ld at sigma = 0, within one rounding of |wl_i| otherwise.
 * Outputs:
 *   token_frames     device i32 [minibatch, maxU-1]  the frame that emits label u; -1 for u >= L.  Non-decreasing in u, equal only
 *                                                    across d = 0 edges.
 *   token_durations  device i32 [minibatch, maxU-1]  the frames label u claims (an element of durations); -1 for u >= L
 *   token_logp       device f32 [minibatch, maxU-1]  see above; 0 for u >= L
 *   scores           device f32 [minibatch]          the best path's log-probability, sigma included; never above -cost of
 *                                                    compute_rnnt_loss_tdt on the same inputs
 * L = 0 is valid (blank edges only).  An utterance without a path (durations {1,2} with L >= T; {0,2} with an odd T) is legitimate
 * data, not an error: score -inf, both integer arrays -1, token_logp 0, never a NaN.  Out-of-range lengths (T < 1, T > maxT, L < 0,
 * L > maxU-1) are device data: they are clamped into the tensor and THAT utterance alone comes back with a NaN score, -1 and 0
 * elsewhere; it reads nothing of the workspace.  Labels outside [0, V) are clamped into it.  A NaN weight never wins a comparison.
 * An utterance's four outputs are BITWISE independent of the rest of the batch, of minibatch, of how the frames were cut into slabs
 * and in which order they were fed, and of the load route (acts_slab 16-byte aligned with V + D a multiple of 4 takes 16-byte
 * loads; anything else scalar loads on the same chunk-to-lane map, the last chunk padded with -inf).
 *
 * Workspace (N = maxT + maxU skewed rows n = t + u, Up = maxU rounded up to 64), in this order, every part 256-byte aligned:
 *   sigma  f32 [1] (padded to 256 bytes)   what the _cells calls were given; _path adds it back for token_logp
 *   w      f32 [minibatch][2 D][N][Up]     plane i = wb_i, plane D + i = wl_i of cell (t,u) at row t + u, column u: the live cells
 *                                          (t < T, u <= L) of the frames a _cells call covers
 *   dec    u8  [minibatch][N][Up]          the decision code of node (t,u) at row t + u, column u; 0xFF: no arrival
 * It never depends on alphabet_size and may hold anything on entry: every value the sweep or the back-trace reads was written by
 * this call sequence's kernels, and the weight of an edge that does not exist is never loaded.
 *
 *   get_rnnt_tdt_align_workspace_size  bytes for (maxT, maxU, minibatch, num_durations).
 *   compute_rnnt_tdt_align_cells   acts_slab f32 [minibatch, slab_frames, maxU, V + D] = the logits of frames frame_offset ...
 *                                  frame_offset + slab_frames - 1 of every utterance: writes the weights of their live cells.
 *   compute_rnnt_tdt_align_path    the sweep over the skewed rows and the back-trace, in one launch, on what a sequence of _cells
 *                                  calls covering frames 0 ... maxT-1 (any order, any slab sizes, the same durations and sigma) has
 *                                  left in the workspace.  The caller passes the SAME durations again.
 *   compute_rnnt_tdt_align         = _cells on the whole tensor (slab_frames = maxT, frame_offset 0) followed by _path.
 * Domain (that of compute_rnnt_loss_tdt): maxU <= 1024, minibatch * maxT * maxU < 2^31, maxT, maxU, minibatch >= 1,
 * 1 <= num_durations <= 8, the duration rule above, sigma >= 0 and finite, alphabet_size >= 2, 0 <= blank_label < alphabet_size
 * (_path takes no alphabet_size: 0 <= blank_label), options.loc == RNNT_GPU, batch_first; 1 <= slab_frames, 0 <= frame_offset,
 * frame_offset + slab_frames <= maxT.  Pointers: none may be NULL; workspace 256-byte aligned, every other device pointer 4-byte
 * aligned.  Anything else: RNNT_STATUS_INVALID_VALUE before anything is enqueued.  Everything is enqueued on options.stream, one
 * launch after the other; no entry point synchronises the host, uses a memset or uses atomics. */
RNNT_API rnntStatus_t get_rnnt_tdt_align_workspace_size(int maxT, int maxU, int minibatch, int num_durations, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_tdt_align_cells(const float *acts_slab, int slab_frames, int frame_offset, const int *flat_labels,
                                                   const int *label_lengths, const int *input_lengths, int alphabet_size,
                                                   const int *durations, int num_durations, float sigma, int minibatch,
                                                   void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_tdt_align_path(int *token_frames, int *token_durations, float *token_logp, float *scores,
                                                  const int *label_lengths, const int *input_lengths, const int *durations,
                                                  int num_durations, int minibatch, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_tdt_align(const float *acts, const int *flat_labels, const int *label_lengths,
                                             const int *input_lengths, int alphabet_size, const int *durations, int num_durations,
                                             float sigma, int minibatch, int *token_frames, int *token_durations, float *token_logp,
                                             float *scores, void *workspace, rnntOptions options);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_TDT_ALIGN_H */
