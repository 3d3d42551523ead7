/* rnnt_lm.h -- n-gram language-model shallow fusion in the beam searches: an extension of include/rnnt.h.
 *
 * include/rnnt.h and libwarprnnt.so are the library's base interface and stay as they are, and so do include/rnnt_bias.h and
 * libwarprnnt_bias.so.  The four entry points declared here are what libwarprnnt_lm.so exports, and all it exports.  The
 * extension library works on the workspaces the base library's begin / feed calls set up, and the base library's results calls
 * read what it wrote: the two share device memory only, neither keeps host state between calls, and both must come from one build.
 */
#ifndef RNNT_LM_H
#define RNNT_LM_H

#include "rnnt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build-only extension: SHALLOW FUSION of a back-off n-gram language model into the four beam searches.  The LM is a
 * deterministic automaton over token ids, as the context graph of include/rnnt_bias.h is; a state stands for a history (the
 * last tokens of the hypothesis, as far as the LM lists them as a context).  It differs from the context graph in two ways: a
 * token the state does not list follows a CHAIN of back-off states, collecting a back-off score at every hop, down to the state
 * of the empty history; and a hypothesis STARTS in the sentence-start context, state 0, which is in general not the empty one.
 * The library ranks candidates inside its kernels and never writes [rows, V] logits, so the LM score is applied there, and the
 * state of a hypothesis travels with it through `parents`.
 *
 * The graph: device arrays, read-only during a decode, described by a host struct.  All scores are already multiplied by the LM
 * weight (natural logarithms times the weight, plus whatever per-token bonus the caller folds in): there is no scale parameter.
 *   arc_offsets   i32 [S + 1]  the arcs of state s are [arc_offsets[s], arc_offsets[s + 1])
 *   arc_tokens    i32 [A]      strictly ascending within a state, in [0, alphabet_size), never the blank
 *   arc_next      i32 [A]      in [0, S)
 *   arc_score     f32 [A]      finite
 *   backoff_next  i32 [S]      backoff_next[E] == E; every chain s, backoff_next[s], ... reaches E in <= RNNT_LM_MAX_HOPS hops
 *   backoff_score f32 [S]      finite, either sign; backoff_score[E] is not read
 * The transition delta(s, v) -> (next, beta), beta an f32, with this ORDER OF f32 ADDITIONS:
 *   v == blank:  (s, 0)
 *   cur = s; hop = 0
 *   loop:
 *     arc (cur, v) listed:  beta = hop == 0 ? arc_score : acc + arc_score;  next = arc_next;  done
 *     cur == E:             beta = hop == 0 ? unk_score : acc + unk_score;  next = E;         done
 *     acc = hop == 0 ? backoff_score[cur] : acc + backoff_score[cur];  cur = backoff_next[cur];  ++hop
 *     hop == RNNT_LM_MAX_HOPS without reaching E: cur = E   (the chain is cut: the result for such a graph is unspecified,
 *                                                            nothing is read out of bounds)
 * The kernels clamp every arc_offsets entry into [0, A] and every arc_next, backoff_next, empty_state and state into [0, S) as
 * they read them: a malformed graph cannot make them index outside the arrays; its results are unspecified.
 *
 * The rules of compute_rnnt_beam_step (include/rnnt.h) with an LM are rules 2' and 3' of include/rnnt_bias.h with this beta.
 * Every hypothesis carries a state q_i: state 0 at begin and after a stream's reset.
 *   2'. per hypothesis i the candidates are the `beam` symbols with the largest f32 key logits_i[v] + beta(q_i, v) (key
 *       descending, symbol ascending; a NaN or -inf key takes no part).  A candidate's score is
 *       s_i + ((double)logits_i[v] - lse_i) + (double)beta.  Ranking across hypotheses, taking, merging and sorting: rules 2 - 5.
 *   3'. the new hypothesis has the state `next` of delta(q_i, v).  Identical sequences have identical states, so a merge keeps
 *       the survivor's.
 * A stream's hypothesis whose token row is full still offers its blank alone (beta = 0).  What the library reports of the MODEL
 * stays raw, without beta: the topk_logits (listed in key order) and lse diagnostics, and the timed searches' per-token
 * log-probability logit - lse.  `scores` include the LM.  The end-of-sentence score is not the library's business: the caller
 * adds it to the scores it reads back, by the states (lm_states).
 *
 * The four entry points are the steps of the same names with two trailing parameters:
 *   graph      host pointer to the struct (device pointers inside); NULL: the call IS the unfused step.  num_states < 1,
 *              num_arcs < 0, empty_state outside [0, S), a non-finite unk_score, a NULL back-off array, or a NULL arc array while
 *              num_arcs > 0: RNNT_STATUS_INVALID_VALUE before anything is enqueued
 *   lm_states  device i32 [minibatch * beam] ([slots * beam]), optional (NULL: not written): the state of every slot after
 *              the step; empty slots are at state 0 and frozen slots keep theirs
 * Begin, feed, results and the workspace sizes are those of the unfused search, unchanged; the state lives in a word of the
 * beam slot that every begin and reset clears (the word the biased steps use: one decode takes an LM or a context graph, not
 * both).  A decode uses the LM step with one and the same graph for ALL of its steps or for none.
 */
#define RNNT_LM_MAX_HOPS 8

typedef struct {
    int num_states;             /* S >= 1; state 0 is where every hypothesis STARTS (sentence start) */
    int num_arcs;               /* A >= 0 */
    int empty_state;            /* E in [0, S): the state of the empty history; the back-off walk ends there; E == 0 is allowed */
    float unk_score;            /* finite: a non-blank token with no arc at E */
    const int *arc_offsets;     /* i32 [S + 1] */
    const int *arc_tokens;      /* i32 [A] strictly ascending within a state, never the blank */
    const int *arc_next;        /* i32 [A] in [0, S) */
    const float *arc_score;     /* f32 [A] finite */
    const int *backoff_next;    /* i32 [S]; backoff_next[E] == E; every chain reaches E in <= RNNT_LM_MAX_HOPS (8) hops */
    const float *backoff_score; /* f32 [S] finite, either sign; backoff_score[E] is not read */
} rnntLmGraph;

RNNT_API rnntStatus_t compute_rnnt_beam_step_lm(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                                int *topk_symbols, float *lse, int joint_size, int alphabet_size, int minibatch,
                                                int beam, int joint_dtype, void *workspace, rnntOptions options,
                                                const rnntLmGraph *graph, int *lm_states);

RNNT_API rnntStatus_t compute_rnnt_beam_timed_step_lm(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                                      int *topk_symbols, float *lse, int joint_size, int alphabet_size,
                                                      int minibatch, int beam, int joint_dtype, void *workspace,
                                                      rnntOptions options, const rnntLmGraph *graph, int *lm_states);

RNNT_API rnntStatus_t compute_rnnt_beam_stream_step_lm(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                                       int *topk_symbols, float *lse, int joint_size, int alphabet_size,
                                                       int slots, int beam, int max_hyp_len, int joint_dtype, void *workspace,
                                                       rnntOptions options, const rnntLmGraph *graph, int *lm_states);

RNNT_API rnntStatus_t compute_rnnt_beam_stream_timed_step_lm(const float *pred_proj, int *parents, int *emitted,
                                                             float *topk_logits, int *topk_symbols, float *lse, int joint_size,
                                                             int alphabet_size, int slots, int beam, int max_hyp_len,
                                                             int joint_dtype, void *workspace, rnntOptions options,
                                                             const rnntLmGraph *graph, int *lm_states);

#ifdef __cplusplus
}
#endif

#endif /* RNNT_LM_H */
