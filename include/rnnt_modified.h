/* rnnt_modified.h -- the modified (one symbol per frame) topology of the transducer loss: an extension of include/rnnt.h.
 *
 * include/rnnt.h and libwarprnnt.so are the library's base interface and stay as they are.  The two entry points declared here
 * are what libwarprnnt_mod.so exports, and all it exports; libwarprnnt.so holds nothing of them.  The extension library is
 * self-contained: it works on a workspace of its own and shares nothing with the base library but the types of rnnt.h.
 */
#ifndef RNNT_MODIFIED_H
#define RNNT_MODIFIED_H

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build-only extension (no upstream counterpart): the MODIFIED topology of the loss -- every frame emits exactly ONE of {blank,
 * next label}, as k2's rnnt_loss(modified=True).  It is the lattice of the paths the beam searches of rnnt.h can produce (they are
 * "modified" beam searches: one symbol per frame); on the standard lattice of compute_rnnt_loss a label edge stays on its frame,
 * so training puts mass -- and FastEmit its push -- on paths that emit several symbols in one frame, which no decoder of this
 * library finds.
 * Per utterance, T = T_b frames, L = L_b labels y_0 ... y_{L-1}, lp(t,u,v) = log_softmax(acts[b,t,u,:])[v], nodes (t,u) with
 * 0 <= t <= T, 0 <= u <= L:
 *   alpha(0,0) = 0, every other alpha(0,u) = -inf
 *   alpha(t,u) = logaddexp(alpha(t-1,u) + lp(t-1,u,blank), alpha(t-1,u-1) + lp(t-1,u-1,y_{u-1}))   (second term for u >= 1)
 *   ln P = alpha(T,L),  costs[b] = -ln P
 *   beta(T,L) = 0, every other beta(T,u) = -inf
 *   beta(t,u) = logaddexp(lp(t,u,blank) + beta(t+1,u), lp(t,u,y_u) + beta(t+1,u+1))                 (second term for u < L)
 * A path consumes all T frames; the last frame may emit a label; there is no mandatory final blank.  Cells (t,u), t < T, u <= L,
 * are live; a path passes through a cell only inside the band u <= t, L - u <= T - t.  With
 *   e_b = exp(alpha(t,u) + lp(t,u,blank) + beta(t+1,u) - ln P),  e_l = exp(alpha(t,u) + lp(t,u,y_u) + beta(t+1,u+1) - ln P)
 *   (e_l = 0 for u = L),  occ = e_b + e_l,
 *   grads[b,t,u,v] = cost_scale[b] ((occ + lambda e_l) softmax(acts[b,t,u,:])[v] - [v == blank] e_b - [v == y_u] (1 + lambda) e_l)
 * -- FastEmit's form of compute_rnnt_loss_fastemit; the costs do not depend on lambda.  Padded cells (t >= T_b or u > L_b) and
 * live cells outside the band get exact zeros and their logits are not read; every element of grads is written.
 * An utterance with L_b > T_b has no path: that is legitimate data, its cost is +inf and all of its gradients are exact zeros,
 * never NaN.  Out-of-range lengths and labels follow the rule of compute_rnnt_loss (clamped; that utterance's cost and the
 * gradients of its clamped lattice are NaN).
 * Numerics.  A row of the lattice depends on the row before it only: the sweeps take T_b steps (the standard ones T_b + L_b
 * diagonals) with every column in flight, alpha and beta side by side in one launch.  The recurrence is carried in float64, the
 * log(1 + e^-|d|) term of a log-add on the float32 units, and alpha / beta are STORED as float64 (at 8 x N(0,1) logits and T = 600
 * their magnitude passes 1e4, where a float32 has 1e-3 of resolution).  The bars of compute_rnnt_loss hold: costs within
 * 1e-4 max(1, |cost|), gradients within 1e-4 |cost_scale| absolute (tests/test_modified_loss_gpu.py; measured values in
 * profiles/modified_topology_notes.md).
 *   workspace      >= get_rnnt_modified_workspace_size() bytes, 256-byte aligned, its own layout (not get_workspace_size's); it
 *                  may hold anything on entry.  The limits of compute_rnnt_loss: maxU <= 8192, minibatch * maxT * maxU < 2^31.
 *   grads == NULL  the forward alone;  costs == NULL  the gradient pass alone, from the workspace a forward left (any number of
 *                  times, with any cost_scale / fastemit_lambda);  both: forward then backward on the caller's stream.
 *   cost_scale     device f32 [minibatch] or NULL (= 1).  fastemit_lambda finite and in [0, 1].
 * RNNT_STATUS_INVALID_VALUE before anything is enqueued: a NULL required pointer (costs and grads both NULL included),
 * alphabet_size < 2, the blank outside [0, alphabet_size), a shape over the limits, a misaligned workspace, a bad fastemit_lambda.
 * The fused joints and the forced aligner keep the standard lattice. */
RNNT_API rnntStatus_t get_rnnt_modified_workspace_size(int maxT, int maxU, int minibatch, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_loss_modified(const float *acts, float *grads, const int *flat_labels,
                                        const int *label_lengths, const int *input_lengths,
                                        const float *cost_scale, int alphabet_size, int minibatch,
                                        float *costs, void *workspace, rnntOptions options, float fastemit_lambda);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_MODIFIED_H */
