// rnnt_bias_entrypoint.hip -- the extern "C" boundary of libwarprnnt_bias.so (declared in include/rnnt_bias.h): the biased steps
// of the four beam searches.  libwarprnnt.so and include/rnnt.h, the base interface, stay as they are.  The base steps'
// argument checks and the body of the graph == NULL forward come from rnnt_decode_host.h, shared with rnnt_entrypoint.hip; this
// unit defines the four twins and nothing else.  build.py links it with the base kernel objects and beam_bias_kernels.hip, and
// rnnt_bias.map exports the four twins alone.
#include "rnnt_decode_host.h"
#include "../../include/rnnt_bias.h"

namespace rnnt {
// beam_kernels.hip
hipError_t launch_beam_step_biased(const float *pred_proj, int *parents, int *emitted, float *topk_logits, int *topk_symbols,
                                   float *lse, int J, int V, int B, int T, int K, int N, int blank, int joint_dtype, bool timed,
                                   void *workspace, hipStream_t s, const rnntBiasGraph *graph, int *bias_states);
}  // namespace rnnt

using namespace rnnt;

extern "C" {

// The biased beam steps (include/rnnt_bias.h): the checks of the step they are twins of, then the graph's; graph == NULL
// is the unbiased entry.  Begin, feed, results and the workspace are those of the unbiased decode.
static rnntStatus_t check_bias(const rnntBiasGraph *g, const int *bias_states) {
    if (g->num_states < 1 || g->num_arcs < 0 || !aligned4(bias_states)) return RNNT_STATUS_INVALID_VALUE;
    if (g->num_arcs > 0 && (!g->arc_offsets || !g->arc_tokens || !g->arc_next || !g->arc_bias || !g->fail_bias))
        return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(g->arc_offsets) || !aligned4(g->arc_tokens) || !aligned4(g->arc_next) || !aligned4(g->arc_bias) ||
        !aligned4(g->fail_bias))
        return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

static rnntStatus_t beam_step_biased(const float *pred_proj, int *parents, int *emitted, float *topk_logits, int *topk_symbols,
                                     float *lse, int joint_size, int alphabet_size, int minibatch, int beam, int joint_dtype,
                                     void *workspace, const rnntOptions &options, bool timed, const rnntBiasGraph *graph,
                                     int *bias_states) {
    if (!pred_proj || !parents || !emitted) return RNNT_STATUS_INVALID_VALUE;
    if (!beam_step_pointers_aligned(pred_proj, parents, emitted, topk_logits, topk_symbols, lse)) return RNNT_STATUS_INVALID_VALUE;
    rnntStatus_t st = check_bias(graph, bias_states);
    if (st != RNNT_STATUS_SUCCESS) return st;
    st = check_beam(options.maxT, joint_size, alphabet_size, minibatch, beam, joint_dtype, workspace, options, timed);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_beam_step_biased(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, joint_size, alphabet_size,
                                     minibatch, options.maxT, beam, options.maxT, options.blank_label, joint_dtype, timed, workspace,
                                     (hipStream_t)options.stream, graph, bias_states));
}

static rnntStatus_t beam_stream_step_biased(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                            int *topk_symbols, float *lse, int joint_size, int alphabet_size, int slots, int beam,
                                            int max_hyp_len, int joint_dtype, void *workspace, const rnntOptions &options, bool timed,
                                            const rnntBiasGraph *graph, int *bias_states) {
    if (!pred_proj || !parents || !emitted) return RNNT_STATUS_INVALID_VALUE;
    if (!beam_step_pointers_aligned(pred_proj, parents, emitted, topk_logits, topk_symbols, lse)) return RNNT_STATUS_INVALID_VALUE;
    rnntStatus_t st = check_bias(graph, bias_states);
    if (st != RNNT_STATUS_SUCCESS) return st;
    st = check_beam_stream(options.maxT, slots, beam, max_hyp_len, 1, joint_size, alphabet_size, joint_dtype, workspace, options, timed);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_beam_step_biased(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, joint_size, alphabet_size, slots,
                                     options.maxT, beam, max_hyp_len, options.blank_label, joint_dtype, timed, workspace,
                                     (hipStream_t)options.stream, graph, bias_states));
}

rnntStatus_t compute_rnnt_beam_step_biased(const float *pred_proj, int *parents, int *emitted, float *topk_logits, int *topk_symbols,
                                           float *lse, int joint_size, int alphabet_size, int minibatch, int beam, int joint_dtype,
                                           void *workspace, rnntOptions options, const rnntBiasGraph *graph, int *bias_states) {
    if (!graph)
        return beam_step_call(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, joint_size, alphabet_size, minibatch, beam,
                              joint_dtype, workspace, options, false);
    return beam_step_biased(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, joint_size, alphabet_size, minibatch, beam,
                            joint_dtype, workspace, options, false, graph, bias_states);
}

rnntStatus_t compute_rnnt_beam_timed_step_biased(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                                 int *topk_symbols, float *lse, int joint_size, int alphabet_size, int minibatch,
                                                 int beam, int joint_dtype, void *workspace, rnntOptions options,
                                                 const rnntBiasGraph *graph, int *bias_states) {
    if (!graph)
        return beam_step_call(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, joint_size, alphabet_size, minibatch, beam,
                              joint_dtype, workspace, options, true);
    return beam_step_biased(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, joint_size, alphabet_size, minibatch, beam,
                            joint_dtype, workspace, options, true, graph, bias_states);
}

rnntStatus_t compute_rnnt_beam_stream_step_biased(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                                  int *topk_symbols, float *lse, int joint_size, int alphabet_size, int slots, int beam,
                                                  int max_hyp_len, int joint_dtype, void *workspace, rnntOptions options,
                                                  const rnntBiasGraph *graph, int *bias_states) {
    if (!graph)
        return beam_stream_step_call(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, joint_size, alphabet_size, slots,
                                     beam, max_hyp_len, joint_dtype, workspace, options, false);
    return beam_stream_step_biased(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, joint_size, alphabet_size, slots, beam,
                                   max_hyp_len, joint_dtype, workspace, options, false, graph, bias_states);
}

rnntStatus_t compute_rnnt_beam_stream_timed_step_biased(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                                        int *topk_symbols, float *lse, int joint_size, int alphabet_size, int slots,
                                                        int beam, int max_hyp_len, int joint_dtype, void *workspace,
                                                        rnntOptions options, const rnntBiasGraph *graph, int *bias_states) {
    if (!graph)
        return beam_stream_step_call(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, joint_size, alphabet_size, slots,
                                     beam, max_hyp_len, joint_dtype, workspace, options, true);
    return beam_stream_step_biased(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, joint_size, alphabet_size, slots, beam,
                                   max_hyp_len, joint_dtype, workspace, options, true, graph, bias_states);
}

}  // extern "C"
