// rnnt_pruned_joint_entrypoint.hip -- the extern "C" boundary of libwarprnnt_prunedjoint.so (declared in include/rnnt_pruned_joint.h):
// the fused joint on a band of S symbols per frame.  build.py links this translation unit with rnnt_pruned_joint_kernels.hip and
// rnnt_pruned_kernels.hip (the lattice sweeps, as libwarprnnt_pruned.so has them), and rnnt_pruned_joint.map keeps everything but
// the two entry points local.  Everything is checked before anything is enqueued, nothing is allocated, everything is enqueued on
// the caller's stream.
#include "../../include/rnnt_pruned_joint.h"
#include "rnnt_pruned_joint.h"
#include "rnnt_host.h"

using namespace rnnt;

// 1 <= s_range <= 64, minibatch * maxT * s_range < 2^31, joint_size a multiple of 64 up to 640
static bool shape_ok(int maxT, int s_range, int minibatch, int joint_size) {
    if (maxT <= 0 || s_range < 1 || s_range > kPrunedMaxS || minibatch <= 0) return false;
    if (joint_size < 64 || joint_size > kPJMaxJ || joint_size % 64 != 0) return false;
    return (long long)minibatch * maxT * s_range < (1ll << 31);
}

extern "C" {

rnntStatus_t get_rnnt_pruned_joint_workspace_size(int maxT, int s_range, int minibatch, int joint_size, size_t *size_bytes) {
    if (!size_bytes || !shape_ok(maxT, s_range, minibatch, joint_size)) return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = make_pruned_joint_layout(maxT, s_range, minibatch, joint_size).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_joint_loss_pruned(const float *enc_proj, const float *pred_proj, const float *W2, const float *b2,
                                            const int *s_begin, const int *flat_labels, const int *label_lengths,
                                            const int *input_lengths, const float *cost_scale, int joint_size, int alphabet_size,
                                            int minibatch, int s_range, int topology, float *costs, float *d_enc_proj,
                                            float *d_pred_proj, float *dW2, float *db2, void *workspace, rnntOptions options,
                                            float fastemit_lambda) {
    if (!(fastemit_lambda >= 0.f && fastemit_lambda <= 1.f)) return RNNT_STATUS_INVALID_VALUE;  // (NaN fails both)
    const int ngrad = (d_enc_proj != nullptr) + (d_pred_proj != nullptr) + (dW2 != nullptr) + (db2 != nullptr);
    if (ngrad != 0 && ngrad != 4) return RNNT_STATUS_INVALID_VALUE;  // all given or all NULL
    if (ngrad == 0 && !costs) return RNNT_STATUS_INVALID_VALUE;
    if (!enc_proj || !pred_proj || !W2 || !b2 || !s_begin || !flat_labels || !label_lengths || !input_lengths || !workspace)
        return RNNT_STATUS_INVALID_VALUE;
    if (!aligned16(enc_proj) || !aligned16(pred_proj) || !aligned16(d_enc_proj) || !aligned16(d_pred_proj)) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(W2) || !aligned4(b2) || !aligned4(dW2) || !aligned4(db2) || !aligned4(costs) || !aligned4(cost_scale) ||
        !aligned4(s_begin) || !aligned4(flat_labels) || !aligned4(label_lengths) || !aligned4(input_lengths))
        return RNNT_STATUS_INVALID_VALUE;
    if (options.loc != RNNT_GPU || !options.batch_first) return RNNT_STATUS_INVALID_VALUE;  // device-only library: no CPU fallback
    if (alphabet_size < 2 || alphabet_size > kPJMaxV || options.blank_label < 0 || options.blank_label >= alphabet_size)
        return RNNT_STATUS_INVALID_VALUE;
    if (topology != RNNT_PRUNED_STANDARD && topology != RNNT_PRUNED_MODIFIED) return RNNT_STATUS_INVALID_VALUE;
    if (options.maxU < 1 || options.maxU > kPrunedMaxU) return RNNT_STATUS_INVALID_VALUE;
    if (!shape_ok(options.maxT, s_range, minibatch, joint_size)) return RNNT_STATUS_INVALID_VALUE;
    if ((long long)minibatch * options.maxU >= (1ll << 31)) return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    const PrunedJointLayout w = make_pruned_joint_layout(options.maxT, s_range, minibatch, joint_size);
    char *ws = (char *)workspace;
    PrunedJointParams p{};
    PrunedParams &q = p.band;
    q.s_begin = s_begin, q.labels = flat_labels, q.label_lengths = label_lengths, q.input_lengths = input_lengths;
    q.cost_scale = cost_scale, q.costs = costs;
    q.lp = (float2 *)(ws + w.band.lp), q.lse = (float *)(ws + w.band.lse);
    q.alpha = (double *)(ws + w.band.alpha), q.edge = (double2 *)(ws + w.band.edge), q.lnP = (double *)(ws + w.band.lnP);
    q.B = minibatch, q.T = options.maxT, q.S = s_range, q.U = options.maxU, q.V = alphabet_size, q.blank = options.blank_label;
    q.topology = topology;
    q.fe_lambda = fastemit_lambda;
    p.enc = enc_proj, p.pred = pred_proj, p.W2 = W2, p.b2 = b2;
    p.d_enc = d_enc_proj, p.d_pred = d_pred_proj, p.dW2 = dW2, p.db2 = db2;
    p.lse_lo = (float *)(ws + w.lse_lo), p.dz = (float *)(ws + w.dz), p.w2max = (unsigned *)(ws + w.w2max);
    p.wpart = (float *)(ws + w.wpart), p.bpart = (float *)(ws + w.bpart);
    p.J = joint_size;
    pruned_joint_geometry(p);
    hipStream_t s = (hipStream_t)options.stream;
    if (costs) {  // the forward: cell kernel, then both sweeps in one launch
        hipError_t e = launch_pruned_joint_forward(p, s);
        if (e != hipSuccess) return from_hip(e);
        e = launch_pruned_sweeps(q, s);
        if (e != hipSuccess) return from_hip(e);
    }
    return ngrad ? from_hip(launch_pruned_joint_backward(p, costs != nullptr, s)) : RNNT_STATUS_SUCCESS;
}

}  // extern "C"
