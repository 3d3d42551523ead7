// rnnt_pruned_entrypoint.hip -- the extern "C" boundary of libwarprnnt_pruned.so (declared in include/rnnt_pruned.h): the loss op on
// a band of S symbols per frame.  build.py links this translation unit with rnnt_pruned_kernels.hip alone, and rnnt_pruned.map
// keeps everything but the two entry points local.  Everything is checked before anything is enqueued, nothing is allocated,
// everything is enqueued on the caller's stream.
#include "../../include/rnnt_pruned.h"
#include "rnnt_pruned.h"
#include "rnnt_host.h"

using namespace rnnt;

// 1 <= s_range <= 64, minibatch * maxT * s_range < 2^31
static bool shape_ok(int maxT, int s_range, int minibatch) {
    if (maxT <= 0 || s_range < 1 || s_range > kPrunedMaxS || minibatch <= 0) return false;
    return (long long)minibatch * maxT * s_range < (1ll << 31);
}

extern "C" {

rnntStatus_t get_rnnt_pruned_workspace_size(int maxT, int s_range, int minibatch, size_t *size_bytes) {
    if (!size_bytes || !shape_ok(maxT, s_range, minibatch)) return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = make_pruned_layout(maxT, s_range, minibatch).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_loss_pruned(const float *acts, float *grads, const int *s_begin, const int *flat_labels,
                                      const int *label_lengths, const int *input_lengths, const float *cost_scale,
                                      int alphabet_size, int minibatch, int s_range, int topology, float *costs, void *workspace,
                                      rnntOptions options, float fastemit_lambda) {
    if (!(fastemit_lambda >= 0.f && fastemit_lambda <= 1.f) || (!grads && !costs)) return RNNT_STATUS_INVALID_VALUE;  // (NaN fails both)
    if (!acts || !s_begin || !flat_labels || !label_lengths || !input_lengths || !workspace) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(acts) || !aligned4(grads) || !aligned4(costs) || !aligned4(cost_scale) || !aligned4(s_begin) ||
        !aligned4(flat_labels) || !aligned4(label_lengths) || !aligned4(input_lengths))
        return RNNT_STATUS_INVALID_VALUE;
    if (options.loc != RNNT_GPU || !options.batch_first) return RNNT_STATUS_INVALID_VALUE;  // device-only library: no CPU fallback
    if (alphabet_size < 2 || options.blank_label < 0 || options.blank_label >= alphabet_size) return RNNT_STATUS_INVALID_VALUE;
    if (topology != RNNT_PRUNED_STANDARD && topology != RNNT_PRUNED_MODIFIED) return RNNT_STATUS_INVALID_VALUE;
    if (options.maxU < 1 || options.maxU > kPrunedMaxU) return RNNT_STATUS_INVALID_VALUE;
    if (!shape_ok(options.maxT, s_range, minibatch)) return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    const PrunedLayout w = make_pruned_layout(options.maxT, s_range, minibatch);
    char *ws = (char *)workspace;
    PrunedParams p{};
    p.acts = acts, p.grads = grads, p.s_begin = s_begin, p.labels = flat_labels;
    p.label_lengths = label_lengths, p.input_lengths = input_lengths;
    p.cost_scale = cost_scale, p.costs = costs;
    p.lp = (float2 *)(ws + w.lp), p.lse = (float *)(ws + w.lse);
    p.alpha = (double *)(ws + w.alpha), p.edge = (double2 *)(ws + w.edge), p.lnP = (double *)(ws + w.lnP);
    p.B = minibatch, p.T = options.maxT, p.S = s_range, p.U = options.maxU, p.V = alphabet_size, p.blank = options.blank_label;
    p.topology = topology;
    p.fe_lambda = fastemit_lambda;
    hipStream_t s = (hipStream_t)options.stream;
    if (costs) {  // the forward: cell pass, then both sweeps in one launch
        hipError_t e = launch_pruned_cells(p, s);
        if (e != hipSuccess) return from_hip(e);
        e = launch_pruned_sweeps(p, s);
        if (e != hipSuccess) return from_hip(e);
    }
    return grads ? from_hip(launch_pruned_grad(p, s)) : RNNT_STATUS_SUCCESS;
}

}  // extern "C"
