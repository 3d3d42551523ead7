// rnnt_tdt_entrypoint.hip -- the extern "C" boundary of libwarprnnt_tdt.so (declared in include/rnnt_tdt.h): the token-and-duration
// (TDT) transducer loss on materialised logits.  libwarprnnt.so and include/rnnt.h, the base interface, stay as they are.  build.py
// links this translation unit with rnnt_tdt_kernels.hip alone, and rnnt_tdt.map keeps everything but the two entry points local.
// Argument validation follows the base library's: everything is checked before anything is enqueued, nothing is allocated,
// everything is enqueued on the caller's stream.
#include "../../include/rnnt_tdt.h"
#include "rnnt_tdt.h"
#include "tdt_host.h"

#include <math.h>

using namespace rnnt;

// the shape limits of this op (include/rnnt_tdt.h): maxU <= 1024, minibatch * maxT * maxU < 2^31, 1 <= num_durations <= 8
static bool shape_ok(int maxT, int maxU, int minibatch, int num_durations) {
    if (maxT <= 0 || maxU <= 0 || maxU > kTdtMaxU || minibatch <= 0) return false;
    if (num_durations < 1 || num_durations > kTdtMaxD) return false;
    return (long long)minibatch * maxT * maxU < (1ll << 31);
}

extern "C" {

rnntStatus_t get_rnnt_tdt_workspace_size(int maxT, int maxU, int minibatch, int num_durations, size_t *size_bytes) {
    if (!size_bytes || !shape_ok(maxT, maxU, minibatch, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = make_tdt_layout(maxT, maxU, minibatch, num_durations).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_loss_tdt(const float *acts, float *grads, const int *flat_labels, const int *label_lengths,
                                   const int *input_lengths, const float *cost_scale, int alphabet_size, const int *durations,
                                   int num_durations, float sigma, int minibatch, float *costs, void *workspace,
                                   rnntOptions options) {
    if (!(sigma >= 0.f) || !isfinite(sigma) || (!grads && !costs)) return RNNT_STATUS_INVALID_VALUE;  // (NaN fails the first)
    if (!acts || !flat_labels || !label_lengths || !input_lengths || !durations || !workspace) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(acts) || !aligned4(grads) || !aligned4(costs) || !aligned4(cost_scale) || !aligned4(flat_labels) ||
        !aligned4(label_lengths) || !aligned4(input_lengths))
        return RNNT_STATUS_INVALID_VALUE;
    if (options.loc != RNNT_GPU || !options.batch_first) return RNNT_STATUS_INVALID_VALUE;  // device-only library: no CPU fallback
    if (alphabet_size < 2 || options.blank_label < 0 || options.blank_label >= alphabet_size) return RNNT_STATUS_INVALID_VALUE;
    if (!shape_ok(options.maxT, options.maxU, minibatch, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    if (!tdt_durations_ok(durations, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    const TdtLayout w = make_tdt_layout(options.maxT, options.maxU, minibatch, num_durations);
    char *ws = (char *)workspace;
    TdtParams p{};
    p.acts = acts, p.grads = grads, p.labels = flat_labels, p.label_lengths = label_lengths, p.input_lengths = input_lengths;
    p.cost_scale = cost_scale, p.costs = costs;
    p.w = (float *)(ws + w.w), p.lse = (float2 *)(ws + w.lse);
    p.alpha = (double *)(ws + w.alpha), p.beta = (double *)(ws + w.beta), p.lnP = (double *)(ws + w.lnP);
    p.B = minibatch, p.T = options.maxT, p.U = options.maxU, p.V = alphabet_size, p.D = num_durations;
    p.blank = options.blank_label;
    p.Up = w.Up, p.N = w.N;
    for (int i = 0; i < kTdtMaxD; ++i) p.dur[i] = i < num_durations ? durations[i] : 0;
    p.sigma = sigma;
    p.divU = make_fastdiv((uint32_t)options.maxU), p.divT = make_fastdiv((uint32_t)options.maxT);
    hipStream_t s = (hipStream_t)options.stream;
    if (costs) {  // the forward: cell pass, then both sweeps in one launch
        hipError_t e = launch_tdt_cells(p, s);
        if (e != hipSuccess) return from_hip(e);
        e = launch_tdt_sweeps(p, s);
        if (e != hipSuccess) return from_hip(e);
    }
    return grads ? from_hip(launch_tdt_grad(p, s)) : RNNT_STATUS_SUCCESS;
}

}  // extern "C"
