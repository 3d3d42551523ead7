// rnnt_simple_entrypoint.hip -- the extern "C" boundary of libwarprnnt_simple.so (declared in include/rnnt_simple.h): the loss op
// of an additive joiner, the first pass of the pruned loss.  build.py links this translation unit with rnnt_simple_kernels.hip
// alone, and rnnt_simple.map keeps everything but the two entry points local.  Everything is checked before anything is enqueued,
// nothing is allocated, everything is enqueued on the caller's stream.
#include "../../include/rnnt_simple.h"
#include "rnnt_simple.h"
#include "rnnt_host.h"

using namespace rnnt;

// 1 <= maxU <= 8192, minibatch * maxT * maxU < 2^31
static bool shape_ok(int maxT, int maxU, int minibatch) {
    if (maxT <= 0 || maxU < 1 || maxU > kSimpleMaxU || minibatch <= 0) return false;
    return (long long)minibatch * maxT * maxU < (1ll << 31);
}

// each of x in [0, 1] and finite (NaN fails both comparisons)
static bool unit(float x) { return x >= 0.f && x <= 1.f; }

extern "C" {

rnntStatus_t get_rnnt_simple_workspace_size(int maxT, int maxU, int minibatch, size_t *size_bytes) {
    if (!size_bytes || !shape_ok(maxT, maxU, minibatch)) return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = make_simple_layout(maxT, maxU, minibatch).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_loss_simple(const float *am, const float *lm, float *grad_am, float *grad_lm, float *occupancy,
                                      const int *flat_labels, const int *label_lengths, const int *input_lengths,
                                      const float *cost_scale, int alphabet_size, int minibatch, int topology,
                                      float lm_only_scale, float am_only_scale, float *costs, void *workspace,
                                      rnntOptions options) {
    if (!unit(lm_only_scale) || !unit(am_only_scale) || !unit(am_only_scale + lm_only_scale)) return RNNT_STATUS_INVALID_VALUE;
    if ((grad_am == nullptr) != (grad_lm == nullptr)) return RNNT_STATUS_INVALID_VALUE;
    if (!costs && !grad_am && !occupancy) return RNNT_STATUS_INVALID_VALUE;  // nothing to compute
    if (!am || !lm || !flat_labels || !label_lengths || !input_lengths || !workspace) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(am) || !aligned4(lm) || !aligned4(grad_am) || !aligned4(grad_lm) || !aligned4(occupancy) || !aligned4(costs) ||
        !aligned4(cost_scale) || !aligned4(flat_labels) || !aligned4(label_lengths) || !aligned4(input_lengths))
        return RNNT_STATUS_INVALID_VALUE;
    if (options.loc != RNNT_GPU || !options.batch_first) return RNNT_STATUS_INVALID_VALUE;  // device-only library: no CPU fallback
    if (alphabet_size < 2 || options.blank_label < 0 || options.blank_label >= alphabet_size) return RNNT_STATUS_INVALID_VALUE;
    if (topology != RNNT_SIMPLE_STANDARD && topology != RNNT_SIMPLE_MODIFIED) return RNNT_STATUS_INVALID_VALUE;
    if (!shape_ok(options.maxT, options.maxU, minibatch)) return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    // the one-dimensional grids of the gradient passes (at least 16 symbols and 16 rows per workgroup): include/rnnt_simple.h
    if (grad_am &&
        (long long)minibatch * ((alphabet_size + 15) / 16) * ((options.maxT + options.maxU + 30) / 16 + 1) >= (1ll << 31))
        return RNNT_STATUS_INVALID_VALUE;
    const SimpleLayout w = make_simple_layout(options.maxT, options.maxU, minibatch);
    char *ws = (char *)workspace;
    SimpleParams p{};
    p.am = am, p.lm = lm, p.grad_am = grad_am, p.grad_lm = grad_lm, p.occupancy = occupancy;
    p.labels = flat_labels, p.label_lengths = label_lengths, p.input_lengths = input_lengths;
    p.cost_scale = cost_scale, p.costs = costs;
    p.lp = (float2 *)(ws + w.lp), p.alpha = (double *)(ws + w.alpha), p.beta = (double *)(ws + w.beta);
    p.Z = (float *)(ws + w.Z), p.e = (float2 *)(ws + w.e), p.Za = (float *)(ws + w.Za), p.Zl = (float *)(ws + w.Zl);
    p.lnP = (double *)(ws + w.lnP);
    p.B = minibatch, p.T = options.maxT, p.U = options.maxU, p.V = alphabet_size, p.blank = options.blank_label;
    p.Up = w.Up, p.NR = w.NR;
    p.skew = topology == RNNT_SIMPLE_STANDARD ? 1 : 0;
    p.a_scale = am_only_scale, p.l_scale = lm_only_scale;
    p.w_scale = fmaxf(0.f, 1.f - (am_only_scale + lm_only_scale));
    hipStream_t s = (hipStream_t)options.stream;
    hipError_t e = hipSuccess;
    if (costs) {  // the forward: row normalisers, cell pass, both sweeps in one launch, occupancies
        if ((e = launch_simple_rows(p, s)) != hipSuccess) return from_hip(e);
        if ((e = launch_simple_cells(p, s)) != hipSuccess) return from_hip(e);
        if ((e = launch_simple_sweeps(p, s)) != hipSuccess) return from_hip(e);
    }
    if (costs || occupancy)  // (without a forward: the occupancies again, from the workspace a forward left, for the caller's buffer)
        if ((e = launch_simple_occupancy(p, s)) != hipSuccess) return from_hip(e);
    return grad_am ? from_hip(launch_simple_grads(p, s)) : RNNT_STATUS_SUCCESS;
}

}  // extern "C"
