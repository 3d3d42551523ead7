/* rnnt_tdt.h -- the token-and-duration (TDT) transducer loss on materialised logits: an extension of include/rnnt.h.
 *
 * include/rnnt.h and libwarprnnt.so are the library's base interface and stay as they are.  The two entry points declared here
 * are what libwarprnnt_tdt.so exports, and all it exports; libwarprnnt.so holds nothing of them.  The extension library is
 * self-contained: it works on a workspace of its own and shares nothing with the base library but the types of rnnt.h.
 */
#ifndef RNNT_TDT_H
#define RNNT_TDT_H

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build-only extension (no upstream counterpart): the loss of the token-and-duration transducer (Xu et al. 2023, "Efficient
 * sequence transduction by jointly predicting tokens and durations").  The joint emits V = alphabet_size token logits and
 * D = num_durations duration logits per cell; an edge of the lattice consumes d frames, d from the duration set.  This text follows
 * the published algorithm; it is not bit-compatible with any other implementation.
 * Per utterance b, T = T_b frames, L = L_b labels y_0 ... y_{L-1}:
 *   acts        device f32 [minibatch, maxT, maxU, V + D], contiguous, maxU = options.maxU.  The first V entries of a cell are the
 *               token logits (blank included), the last D the duration logits.
 *   durations   HOST int [D], read during the call: strictly increasing, durations[0] in {0, 1}, some d > 0 present,
 *               1 <= D <= 8, durations[D-1] <= 8.
 *   lp(t,u,v) = log_softmax(acts[b,t,u,:V])[v],  ld(t,u,i) = log_softmax(acts[b,t,u,V:])[i]   -- two separate log-softmaxes
 *   sigma       >= 0, finite: the logit under-normalisation; it applies to the tokens only.
 * Lattice.  Nodes (t,u), 0 <= t < T, 0 <= u <= L, and the terminal node (T, L).  From (t,u), for each i with d = durations[i]:
 *   blank edge to (t+d, u),    weight wb_i = lp(t,u,blank) - sigma + ld(t,u,i);  it exists iff d > 0 and (t+d < T, or t+d == T and u == L)
 *   label edge to (t+d, u+1),  weight wl_i = lp(t,u,y_u)  - sigma + ld(t,u,i);  it exists iff u < L and t+d < T
 * A path ends with a blank edge that lands exactly on t + d = T; overshooting T is not allowed and a label edge never lands on T.
 *   alpha(0,0) = 0; any other alpha(node) = logsumexp over incoming edges of alpha(source) + w
 *   ln P = alpha(T,L),  costs[b] = -ln P
 *   beta(T,L) = 0;  beta(t,u) = logsumexp over outgoing edges of w + beta(target)
 * Gradients.  Per cell, with e(edge) = exp(alpha(t,u) + w + beta(target) - ln P):
 *   g_b = sum of e over the blank edges, g_l = over the label edges, g_i = over both kinds of edge of duration i, m = g_b + g_l,
 *   cs = cost_scale[b] (1 when cost_scale is NULL):
 *   grads[b,t,u,v]     = cs (m softmax(acts[b,t,u,:V])[v] - [v == blank] g_b - [u < L and v == y_u] g_l)     v < V
 *   grads[b,t,u,V + i] = cs (m softmax(acts[b,t,u,V:])[i] - g_i)
 * -- the exact derivative of costs[b], sigma included.
 * Every element of grads is written.  The logits of a cell are streamed once by the forward and once by the gradient pass (the
 * forward reads a cell's blank, label and duration logits a second time, from cache).  Padded cells (t >= T_b or u > L_b) get
 * exact zeros and their logits are not read.  Cells no path crosses (alpha = -inf, or every target's beta = -inf) get exact
 * zeros, never NaN.  An utterance without a path is legitimate data (durations {0,2} with odd T; {1,2} with L >= T): its cost is
 * +inf and all of its gradients are exact zeros.
 * Out-of-range lengths and labels follow the rule of compute_rnnt_loss (clamped; that utterance's cost and the gradients of its
 * clamped lattice are NaN for out-of-range lengths).
 * Numerics.  A lattice row depends on up to dmax + 1 earlier rows (dmax = durations[D-1]), and a label edge with d = 0 stays on
 * its frame: the sweeps walk the T_b + L_b + 1 skewed rows n = t + u with every column in flight, alpha and beta side by side in
 * one launch, and keep the last dmax + 2 rows on chip.  The recurrence is carried in float64; the logsumexp over the up to 2 D
 * edges is a max followed by a sum of exponentials in the order of i (blank, label), the exponentials and the logarithm on the
 * float32 units; alpha and beta are STORED as float64.  The normalisers of a cell are float32, from the float32 logits (running
 * max / sum of exponentials).  The bars of compute_rnnt_loss hold: costs within 1e-4 max(1, |cost|), gradients within
 * 1e-4 |cost_scale| absolute (tests/test_tdt_loss_gpu.py; measured values in profiles/tdt_loss_notes.md).
 * Single stream, no memset, no atomics: two calls on the same input give the same bits, and an utterance's results do not depend
 * on the batch around it.
 *   workspace      >= get_rnnt_tdt_workspace_size() bytes, 256-byte aligned, its own layout; it may hold anything on entry.
 *                  Limits: maxU <= 1024 (one lattice column per thread of the sweep), minibatch * maxT * maxU < 2^31.
 *   grads == NULL  the forward alone;  costs == NULL  the gradient pass alone, from the workspace a forward left (any number of
 *                  times, with any cost_scale).  The caller passes the SAME durations and sigma again: the workspace's layout
 *                  depends on num_durations and the gradient pass reads the duration set.  Both given: forward then backward on
 *                  the caller's stream (options.stream).
 *   cost_scale     device f32 [minibatch] or NULL (= 1).
 * RNNT_STATUS_INVALID_VALUE before anything is enqueued: a NULL required pointer (costs and grads both NULL included),
 * alphabet_size < 2, the blank outside [0, alphabet_size), a durations array that breaks the rule above, a sigma that is negative
 * or not finite, a workspace that is not 256-byte aligned, minibatch * maxT * maxU >= 2^31, maxU > 1024, maxT, maxU or minibatch
 * < 1, num_durations outside [1, 8]; and, as in compute_rnnt_loss, options.loc != RNNT_GPU (there is no CPU path),
 * options.batch_first == false, and acts, grads, costs, cost_scale, flat_labels, label_lengths or input_lengths not 4-byte aligned.
 * get_rnnt_tdt_workspace_size returns it for a NULL size_bytes and for the same shape limits. */
RNNT_API rnntStatus_t get_rnnt_tdt_workspace_size(int maxT, int maxU, int minibatch, int num_durations, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_loss_tdt(const float *acts, float *grads, const int *flat_labels, const int *label_lengths,
                                            const int *input_lengths, const float *cost_scale, int alphabet_size,
                                            const int *durations, int num_durations, float sigma, int minibatch,
                                            float *costs, void *workspace, rnntOptions options);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_TDT_H */
