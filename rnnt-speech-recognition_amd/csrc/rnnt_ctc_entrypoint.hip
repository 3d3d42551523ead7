// rnnt_ctc_entrypoint.hip -- the extern "C" boundary of libwarprnnt_ctc.so (declared in include/rnnt_ctc.h): the CTC loss and the
// greedy CTC decoder of the auxiliary head.  libwarprnnt.so and include/rnnt.h, the base interface, stay as they are.  build.py
// links this translation unit with rnnt_ctc_kernels.hip alone, and rnnt_ctc.map keeps everything but the three entry points local.
// Argument validation follows the base library's: everything is checked before anything is enqueued, nothing is allocated,
// everything is enqueued on the caller's stream.
#include "../../include/rnnt_ctc.h"
#include "rnnt_ctc.h"
#include "rnnt_host.h"

using namespace rnnt;

// the shape limits of the loss: maxU in [1, 8192], minibatch * maxT * (2 maxU - 1) < 2^31
static bool shape_ok(int maxT, int maxU, int minibatch) {
    if (maxT <= 0 || maxU <= 0 || maxU > kMaxU || minibatch <= 0) return false;
    return (long long)minibatch * maxT * (2ll * maxU - 1) < (1ll << 31);
}

// minibatch * maxT * alphabet_size < 2^31
static bool acts_ok(int maxT, int minibatch, int alphabet_size) {
    if (maxT <= 0 || minibatch <= 0) return false;
    return (long long)minibatch * maxT * alphabet_size < (1ll << 31);
}

extern "C" {

rnntStatus_t get_rnnt_ctc_workspace_size(int maxT, int maxU, int minibatch, size_t *size_bytes) {
    if (!size_bytes || !shape_ok(maxT, maxU, minibatch)) return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = make_ctc_layout(maxT, maxU, minibatch).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_ctc_loss(const float *acts, float *grads, const int *flat_labels, const int *label_lengths,
                                   const int *input_lengths, const float *cost_scale, int alphabet_size, int minibatch,
                                   float *costs, void *workspace, rnntOptions options) {
    if (!grads && !costs) return RNNT_STATUS_INVALID_VALUE;
    if (!acts || !flat_labels || !label_lengths || !input_lengths || !workspace) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(acts) || !aligned4(grads) || !aligned4(costs) || !aligned4(cost_scale) || !aligned4(flat_labels) ||
        !aligned4(label_lengths) || !aligned4(input_lengths))
        return RNNT_STATUS_INVALID_VALUE;
    if (options.loc != RNNT_GPU || !options.batch_first) return RNNT_STATUS_INVALID_VALUE;  // device-only library: no CPU fallback
    if (alphabet_size < 2 || options.blank_label < 0 || options.blank_label >= alphabet_size) return RNNT_STATUS_INVALID_VALUE;
    if (!shape_ok(options.maxT, options.maxU, minibatch) || !acts_ok(options.maxT, minibatch, alphabet_size))
        return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    const CtcLayout w = make_ctc_layout(options.maxT, options.maxU, minibatch);
    char *ws = (char *)workspace;
    CtcParams p{};
    p.acts = acts, p.grads = grads, p.labels = flat_labels, p.label_lengths = label_lengths, p.input_lengths = input_lengths;
    p.cost_scale = cost_scale, p.costs = costs;
    p.lpa = (float2 *)(ws + w.lpa), p.lpb = (float2 *)(ws + w.lpb), p.lse = (float *)(ws + w.lse);
    p.alpha = (double2 *)(ws + w.alpha), p.beta = (double2 *)(ws + w.beta), p.lnP = (double *)(ws + w.lnP);
    p.meta = (int *)(ws + w.meta), p.lab = (int *)(ws + w.lab), p.flags = (int *)(ws + w.flags);
    p.B = minibatch, p.T = options.maxT, p.U = options.maxU, p.V = alphabet_size, p.blank = options.blank_label;
    p.Up = w.Up;
    hipStream_t s = (hipStream_t)options.stream;
    if (costs) {  // the forward: the labels' tables, the row pass, then both sweeps in one launch
        hipError_t e = launch_ctc_prepare(p, s);
        if (e != hipSuccess) return from_hip(e);
        e = launch_ctc_rows(p, s);
        if (e != hipSuccess) return from_hip(e);
        e = launch_ctc_sweeps(p, s);
        if (e != hipSuccess) return from_hip(e);
    }
    return grads ? from_hip(launch_ctc_grad(p, s)) : RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_ctc_greedy(const float *acts, const int *input_lengths, int alphabet_size, int minibatch, int *tokens,
                                     int *token_frames, int *lengths, rnntOptions options) {
    if (!acts || !input_lengths || !tokens || !lengths) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(acts) || !aligned4(input_lengths) || !aligned4(tokens) || !aligned4(token_frames) || !aligned4(lengths))
        return RNNT_STATUS_INVALID_VALUE;
    if (options.loc != RNNT_GPU || !options.batch_first) return RNNT_STATUS_INVALID_VALUE;
    if (alphabet_size < 2 || options.blank_label < 0 || options.blank_label >= alphabet_size) return RNNT_STATUS_INVALID_VALUE;
    if (!acts_ok(options.maxT, minibatch, alphabet_size)) return RNNT_STATUS_INVALID_VALUE;
    CtcGreedyParams p{};
    p.acts = acts, p.input_lengths = input_lengths, p.tokens = tokens, p.token_frames = token_frames, p.lengths = lengths;
    p.B = minibatch, p.T = options.maxT, p.V = alphabet_size, p.blank = options.blank_label;
    return from_hip(launch_ctc_greedy(p, (hipStream_t)options.stream));
}

}  // extern "C"
