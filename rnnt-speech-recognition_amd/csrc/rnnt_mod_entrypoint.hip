// rnnt_mod_entrypoint.hip -- the extern "C" boundary of libwarprnnt_mod.so (declared in include/rnnt_modified.h): the loss op on the
// modified (one symbol per frame) lattice.  libwarprnnt.so and include/rnnt.h, the base interface, stay as they are.  build.py
// links this translation unit with rnnt_mod_kernels.hip alone, and rnnt_mod.map keeps everything but the two entry points local.
// Argument validation follows the base library's: everything is checked before anything is enqueued, nothing is allocated,
// everything is enqueued on the caller's stream.
#include "../../include/rnnt_modified.h"
#include "rnnt_mod.h"
#include "rnnt_host.h"

using namespace rnnt;

// the shape limits of the op (include/rnnt.h): maxU <= 8192, minibatch * maxT * maxU < 2^31
static bool shape_ok(int maxT, int maxU, int minibatch) {
    if (maxT <= 0 || maxU <= 0 || maxU > kMaxU || minibatch <= 0) return false;
    return (long long)minibatch * maxT * maxU < (1ll << 31);
}

extern "C" {

rnntStatus_t get_rnnt_modified_workspace_size(int maxT, int maxU, int minibatch, size_t *size_bytes) {
    if (!size_bytes || !shape_ok(maxT, maxU, minibatch)) return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = make_mod_layout(maxT, maxU, minibatch).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_loss_modified(const float *acts, float *grads, const int *flat_labels, const int *label_lengths,
                                        const int *input_lengths, const float *cost_scale, int alphabet_size, int minibatch,
                                        float *costs, void *workspace, rnntOptions options, float fastemit_lambda) {
    if (!(fastemit_lambda >= 0.f && fastemit_lambda <= 1.f) || (!grads && !costs)) return RNNT_STATUS_INVALID_VALUE;  // (NaN fails both)
    if (!acts || !flat_labels || !label_lengths || !input_lengths || !workspace) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(acts) || !aligned4(grads) || !aligned4(costs) || !aligned4(cost_scale) || !aligned4(flat_labels) ||
        !aligned4(label_lengths) || !aligned4(input_lengths))
        return RNNT_STATUS_INVALID_VALUE;
    if (options.loc != RNNT_GPU || !options.batch_first) return RNNT_STATUS_INVALID_VALUE;  // device-only library: no CPU fallback
    if (alphabet_size < 2 || options.blank_label < 0 || options.blank_label >= alphabet_size) return RNNT_STATUS_INVALID_VALUE;
    if (!shape_ok(options.maxT, options.maxU, minibatch)) return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    const ModLayout w = make_mod_layout(options.maxT, options.maxU, minibatch);
    char *ws = (char *)workspace;
    ModParams p{};
    p.acts = acts, p.grads = grads, p.labels = flat_labels, p.label_lengths = label_lengths, p.input_lengths = input_lengths;
    p.cost_scale = cost_scale, p.costs = costs;
    p.lp = (float2 *)(ws + w.lp), p.lse = (float *)(ws + w.lse);
    p.alpha = (double *)(ws + w.alpha), p.beta = (double *)(ws + w.beta), p.lnP = (double *)(ws + w.lnP);
    p.B = minibatch, p.T = options.maxT, p.U = options.maxU, p.V = alphabet_size, p.blank = options.blank_label;
    p.Up = w.Up;
    p.fe_lambda = fastemit_lambda;
    p.divU = make_fastdiv((uint32_t)options.maxU), p.divT = make_fastdiv((uint32_t)options.maxT);
    hipStream_t s = (hipStream_t)options.stream;
    if (costs) {  // the forward: cell pass, then both sweeps in one launch
        hipError_t e = launch_mod_cells(p, s);
        if (e != hipSuccess) return from_hip(e);
        e = launch_mod_sweeps(p, s);
        if (e != hipSuccess) return from_hip(e);
    }
    return grads ? from_hip(launch_mod_grad(p, s)) : RNNT_STATUS_SUCCESS;
}

}  // extern "C"
