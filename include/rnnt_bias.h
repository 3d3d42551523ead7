/* rnnt_bias.h -- contextual biasing of the beam searches: an extension of include/rnnt.h.
 *
 * include/rnnt.h and libwarprnnt.so are the library's base interface and stay as they are.  The four entry points declared here
 * are what libwarprnnt_bias.so exports, and all it exports; libwarprnnt.so holds nothing of them.  The extension library works on
 * the workspaces the base library's begin / feed calls set up, and the base library's results calls read what it wrote: the two
 * share device memory only, neither keeps host state between calls, and both must come from one build.
 */
#ifndef RNNT_BIAS_H
#define RNNT_BIAS_H

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build-only extension: CONTEXTUAL BIASING (hotword boosting) for the four beam searches.  A context graph is a deterministic
 * automaton over token ids, as the k2 / icefall recipes build it from a list of phrases: a hypothesis that spells out a listed
 * phrase collects a bonus arc by arc, and gives back what it has not earned when the match breaks off.  The library ranks
 * candidates inside its kernels and never writes [rows, V] logits, so the bonus is applied there, and the automaton state of a
 * hypothesis travels with it through `parents`.
 *
 * The graph: device arrays, read-only during a decode, described by a host struct.  State 0 is the root.
 *   arc_offsets i32 [S + 1]  the arcs of state s are [arc_offsets[s], arc_offsets[s + 1])
 *   arc_tokens  i32 [A]      strictly ascending within a state, in [0, alphabet_size), never the blank
 *   arc_next    i32 [A]      in [0, S)
 *   arc_bias    f32 [A]      finite
 *   fail_bias   f32 [S]      finite, <= 0, fail_bias[0] == 0
 * The transition delta(s, v) -> (next, beta), beta an f32:
 *   v == blank                                   (s, 0)
 *   arc (s, v) is listed                         (arc_next, arc_bias)
 *   otherwise, s != 0 and arc (0, v) is listed   (arc_next of that root arc, fail_bias[s] + arc_bias of it: one f32 addition)
 *   otherwise                                    (0, fail_bias[s])
 * The kernels clamp every arc_offsets entry into [0, A] and every arc_next and state into [0, S) as they read them: a malformed
 * graph cannot make them index outside the arrays; its results are unspecified.
 *
 * The rules of compute_rnnt_beam_step (include/rnnt.h) with a graph.  Every hypothesis carries a state q_i: the root at begin and after a stream's
 * reset.
 *   2'. per hypothesis i the candidates are the `beam` symbols with the largest f32 key logits_i[v] + beta(q_i, v) (key
 *       descending, symbol ascending; a NaN or -inf key takes no part).  A candidate's score is
 *       s_i + ((double)logits_i[v] - lse_i) + (double)beta.  Ranking across hypotheses, taking, merging and sorting: rules 2 - 5.
 *   3'. the new hypothesis has the state `next` of delta(q_i, v).  Identical sequences have identical states, so a merge keeps
 *       the survivor's.
 * A stream's hypothesis whose token row is full still offers its blank alone (beta = 0).  What the library reports of the MODEL
 * stays raw, without beta: the topk_logits (listed in key order) and lse diagnostics, and the timed searches' per-token
 * log-probability logit - lse.  `scores` include the bias.  Unlike rule 2 -- where the `beam` best logits of a hypothesis are
 * also its `beam` best candidates -- rule 2' is a pruning rule of its own: the per-hypothesis candidates are chosen by the key.
 *
 * The four entry points are the steps of the same names with two trailing parameters:
 *   graph        host pointer to the struct (device pointers inside); NULL: the call IS the unbiased step.  num_states < 1,
 *                num_arcs < 0, or a NULL array while num_arcs > 0: RNNT_STATUS_INVALID_VALUE before anything is enqueued
 *   bias_states  device i32 [minibatch * beam] ([slots * beam]), optional (NULL: not written): the state of every slot after
 *                the step; empty slots are at the root and frozen slots keep theirs
 * Begin, feed, results and the workspace sizes are those of the unbiased search, unchanged; the state lives in a word of the
 * beam slot that every begin and reset clears.  A decode uses the biased step with one and the same graph for ALL of its steps
 * or for none: an unbiased step in between returns every state to the root.
 */
typedef struct {
    int num_states;           /* S >= 1; state 0 is the root */
    int num_arcs;             /* A >= 0 */
    const int *arc_offsets;   /* i32 [S + 1] */
    const int *arc_tokens;    /* i32 [A] */
    const int *arc_next;      /* i32 [A] */
    const float *arc_bias;    /* f32 [A] */
    const float *fail_bias;   /* f32 [S] */
} rnntBiasGraph;

RNNT_API rnntStatus_t compute_rnnt_beam_step_biased(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                                    int *topk_symbols, float *lse, int joint_size, int alphabet_size, int minibatch,
                                                    int beam, int joint_dtype, void *workspace, rnntOptions options,
                                                    const rnntBiasGraph *graph, int *bias_states);

RNNT_API rnntStatus_t compute_rnnt_beam_timed_step_biased(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                                          int *topk_symbols, float *lse, int joint_size, int alphabet_size,
                                                          int minibatch, int beam, int joint_dtype, void *workspace,
                                                          rnntOptions options, const rnntBiasGraph *graph, int *bias_states);

RNNT_API rnntStatus_t compute_rnnt_beam_stream_step_biased(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                                           int *topk_symbols, float *lse, int joint_size, int alphabet_size,
                                                           int slots, int beam, int max_hyp_len, int joint_dtype, void *workspace,
                                                           rnntOptions options, const rnntBiasGraph *graph, int *bias_states);

RNNT_API rnntStatus_t compute_rnnt_beam_stream_timed_step_biased(const float *pred_proj, int *parents, int *emitted,
                                                                 float *topk_logits, int *topk_symbols, float *lse, int joint_size,
                                                                 int alphabet_size, int slots, int beam, int max_hyp_len,
                                                                 int joint_dtype, void *workspace, rnntOptions options,
                                                                 const rnntBiasGraph *graph, int *bias_states);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_BIAS_H */
