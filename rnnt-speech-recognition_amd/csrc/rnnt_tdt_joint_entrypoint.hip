// rnnt_tdt_joint_entrypoint.hip -- the extern "C" boundary of libwarprnnt_tdtjoint.so (declared in include/rnnt_tdt_joint.h): the
// TDT loss with the joint network inside.  build.py links this translation unit with rnnt_tdt_joint_kernels.hip and
// rnnt_tdt_kernels.hip (the lattice sweeps, as libwarprnnt_tdt.so has them), and rnnt_tdt_joint.map keeps everything but the two
// entry points local.  Everything is checked before anything is enqueued, nothing is allocated, everything is enqueued on the
// caller's stream.
#include "../../include/rnnt_tdt_joint.h"
#include "rnnt_tdt_joint.h"
#include "tdt_host.h"

#include <math.h>

using namespace rnnt;

// the lattice limits of rnnt_tdt.h (maxU <= 1024, minibatch * maxT * maxU < 2^31, 1 <= num_durations <= 8) and the joint's
// (joint_size a multiple of 64 up to 640)
static bool shape_ok(int maxT, int maxU, int minibatch, int num_durations, int joint_size) {
    if (maxT <= 0 || maxU <= 0 || maxU > kTdtMaxU || minibatch <= 0) return false;
    if (num_durations < 1 || num_durations > kTdtMaxD) return false;
    if (joint_size < 64 || joint_size > kTJMaxJ || joint_size % 64 != 0) return false;
    return (long long)minibatch * maxT * maxU < (1ll << 31);
}

extern "C" {

rnntStatus_t get_rnnt_tdt_joint_workspace_size(int maxT, int maxU, int minibatch, int num_durations, int joint_size, size_t *size_bytes) {
    if (!size_bytes || !shape_ok(maxT, maxU, minibatch, num_durations, joint_size)) return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = make_tdt_joint_layout(maxT, maxU, minibatch, num_durations, joint_size).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_joint_loss_tdt(const float *enc_proj, const float *pred_proj, const float *W2, const float *b2,
                                         const int *flat_labels, const int *label_lengths, const int *input_lengths,
                                         const float *cost_scale, int joint_size, int alphabet_size, const int *durations,
                                         int num_durations, float sigma, int minibatch, float *costs, float *d_enc_proj,
                                         float *d_pred_proj, float *dW2, float *db2, void *workspace, rnntOptions options) {
    if (!(sigma >= 0.f) || !isfinite(sigma)) return RNNT_STATUS_INVALID_VALUE;  // (NaN fails the first)
    const int ngrad = (d_enc_proj != nullptr) + (d_pred_proj != nullptr) + (dW2 != nullptr) + (db2 != nullptr);
    if (ngrad != 0 && ngrad != 4) return RNNT_STATUS_INVALID_VALUE;  // all given or all NULL
    if (ngrad == 0 && !costs) return RNNT_STATUS_INVALID_VALUE;
    if (!enc_proj || !pred_proj || !W2 || !b2 || !flat_labels || !label_lengths || !input_lengths || !durations || !workspace)
        return RNNT_STATUS_INVALID_VALUE;
    if (!aligned16(enc_proj) || !aligned16(pred_proj) || !aligned16(d_enc_proj) || !aligned16(d_pred_proj)) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(W2) || !aligned4(b2) || !aligned4(dW2) || !aligned4(db2) || !aligned4(costs) || !aligned4(cost_scale) ||
        !aligned4(flat_labels) || !aligned4(label_lengths) || !aligned4(input_lengths))
        return RNNT_STATUS_INVALID_VALUE;
    if (options.loc != RNNT_GPU || !options.batch_first) return RNNT_STATUS_INVALID_VALUE;  // device-only library: no CPU fallback
    if (!shape_ok(options.maxT, options.maxU, minibatch, num_durations, joint_size)) return RNNT_STATUS_INVALID_VALUE;
    if (alphabet_size < 2 || alphabet_size > kTJMaxR - num_durations || options.blank_label < 0 || options.blank_label >= alphabet_size)
        return RNNT_STATUS_INVALID_VALUE;
    if (!tdt_durations_ok(durations, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    const TdtJointLayout w = make_tdt_joint_layout(options.maxT, options.maxU, minibatch, num_durations, joint_size);
    char *ws = (char *)workspace;
    TdtJointParams p{};
    TdtParams &q = p.lat;
    q.labels = flat_labels, q.label_lengths = label_lengths, q.input_lengths = input_lengths;
    q.cost_scale = cost_scale, q.costs = costs;
    q.w = (float *)(ws + w.lat.w), q.lse = (float2 *)(ws + w.lat.lse);
    q.alpha = (double *)(ws + w.lat.alpha), q.beta = (double *)(ws + w.lat.beta), q.lnP = (double *)(ws + w.lat.lnP);
    q.B = minibatch, q.T = options.maxT, q.U = options.maxU, q.V = alphabet_size, q.D = num_durations;
    q.blank = options.blank_label;
    q.Up = w.lat.Up, q.N = w.lat.N;
    for (int i = 0; i < kTdtMaxD; ++i) q.dur[i] = i < num_durations ? durations[i] : 0;
    q.sigma = sigma;
    q.divU = make_fastdiv((uint32_t)options.maxU), q.divT = make_fastdiv((uint32_t)options.maxT);
    p.enc = enc_proj, p.pred = pred_proj, p.W2 = W2, p.b2 = b2;
    p.d_enc = d_enc_proj, p.d_pred = d_pred_proj, p.dW2 = dW2, p.db2 = db2;
    p.lse_lo = (float2 *)(ws + w.lse_lo), p.occ = (float *)(ws + w.occ);
    p.encpart = (float *)(ws + w.encpart), p.predpart = (float *)(ws + w.predpart);
    p.w2max = (unsigned *)(ws + w.w2max), p.wpart = (float *)(ws + w.wpart), p.bpart = (float *)(ws + w.bpart);
    p.J = joint_size;
    tdt_joint_geometry(p);
    hipStream_t s = (hipStream_t)options.stream;
    if (costs) {  // the forward: cell kernel, then both sweeps in one launch
        hipError_t e = launch_tdt_joint_forward(p, s);
        if (e != hipSuccess) return from_hip(e);
        e = launch_tdt_sweeps(q, s);
        if (e != hipSuccess) return from_hip(e);
    }
    return ngrad ? from_hip(launch_tdt_joint_backward(p, costs != nullptr, s)) : RNNT_STATUS_SUCCESS;
}

}  // extern "C"
