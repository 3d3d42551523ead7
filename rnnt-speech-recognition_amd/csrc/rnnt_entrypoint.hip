// rnnt_entrypoint.hip -- the extern "C" boundary of libwarprnnt.so (declared in include/rnnt.h).
//
// Replaces the reference's native entry points (warp-transducer `src/rnnt_entrypoint.cu`, named at
// cmake/warp-rnnt-cmakelist.txt:99; reached from utils/loss.py:34-35).  Argument validation follows
// the published contract: null pointers / non-positive sizes ->
// RNNT_STATUS_INVALID_VALUE; nothing is allocated; everything is enqueued on the caller's stream.
#include "../../include/rnnt.h"
#include "rnnt_common.h"
#include "rnnt_lin.h"
#include "rnnt_align.h"
#include "rnnt_decode_host.h"

using namespace rnnt;

namespace rnnt {
// joint_kernels.hip
hipError_t joint_workspace_bytes(int T, int U, int B, int J, int V, int joint_dtype, size_t *bytes);
hipError_t joint_f16_backward_rows(void *workspace, int T, int U, int B, int J, int V, int rows[2], hipStream_t s);
hipError_t joint_backward_rows(void *workspace, int T, int U, int B, int J, int V, int rows[2], hipStream_t s);
hipError_t launch_joint_loss(const float *enc_proj, const float *pred_proj, const float *W2, const float *b2,
                             const int *labels, const int *label_lengths, const int *input_lengths,
                             const float *cost_scale, int J, int V, int B, int T, int U, int blank, float *costs,
                             float *d_enc_proj, float *d_pred_proj, float *dW2, float *db2, int joint_dtype,
                             int phases, void *workspace, hipStream_t s, const JointHooks *hooks, float fe_lambda);
hipError_t joint_aux_pointers(void *workspace, int T, int U, int B, int J, int V, float **expE, float **expP, float **tflag);
hipError_t launch_joint_prefill(void *workspace, int T, int U, int B, int J, int V, hipStream_t s);
bool joint_dtype_supported(int joint_dtype, int J, int V);
// dense_kernels.hip (the joint's first Dense layer)
bool dense_supported(int H, int J);
hipError_t dense_workspace_bytes(int B, int T, int U, int H, int J, size_t base, size_t *bytes);
void dense_proj_pointers(void *workspace, int B, int T, int U, int H, int J, size_t base, float **enc_proj, float **pred_proj,
                         float **d_enc_proj, float **d_pred_proj);
void dense_hook_pointers(void *workspace, int B, int T, int U, int H, int J, size_t base, unsigned **dmax_enc, unsigned **dmax_pred);
hipError_t launch_dense_fwd(const float *enc, const float *pred, const float *W1, const float *b1, int B, int T, int U, int H, int J,
                            void *workspace, size_t base, float *expE, float *expP, float *tflag, hipStream_t s);
hipError_t launch_dense_bwd(int B, int T, int U, int H, int J, float *d_enc, float *d_pred, float *dW1, float *db1, void *workspace,
                            size_t base, hipStream_t s);
hipError_t launch_joint_logits(const float *enc_proj, const float *pred_proj, const float *W2, const float *b2, int J, int V,
                               int B, int T, int U, float *logits, void *workspace, hipStream_t s);
// joint_f16_kernels.hip
hipError_t joint_f16_workspace_bytes(int T, int U, int B, int J, int V, size_t *bytes);
hipError_t launch_joint_logits_f16(const float *enc_proj, const float *pred_proj, const float *W2, const float *b2, int J, int V,
                                   int B, int T, int U, float *logits, void *workspace, hipStream_t s);
// prednet_kernels.hip (the prediction-network step of the decoders)
bool prednet_layout_ok(const rnntPrednetBlock *blocks, int L, int E, int V, int Jp, int R, size_t *bytes);
hipError_t launch_prednet_begin(const float *emb, const rnntPrednetBlock *blocks, int L, int E, int V, const float *W1, int Jp, int R,
                                float *out, void *workspace, hipStream_t s);
hipError_t launch_prednet_step(const int *emitted, const int *parents, float *out, const rnntPrednetBlock *blocks, int L, int E,
                               int V, int Jp, int R, void *workspace, hipStream_t s);
hipError_t launch_prednet_reset(const int *reset, float *out, const rnntPrednetBlock *blocks, int L, int E, int V, int Jp, int R,
                                void *workspace, hipStream_t s);
// encoder_kernels.hip (the encoder's forward pass, state carried across runs)
bool encoder_layout_ok(const rnntPrednetBlock *blocks, int L, int F, float bn_eps, int ridx, int f, int R, int Tmax, size_t *bytes);
hipError_t launch_encoder_begin(const rnntPrednetBlock *blocks, int L, int F, const float *bn_mean, const float *bn_var,
                                const float *bn_weight, const float *bn_bias, float bn_eps, int ridx, int f, int R, int Tmax,
                                void *workspace, hipStream_t s);
hipError_t launch_encoder_run(const float *x, int T, float *out, const rnntPrednetBlock *blocks, int L, int F, float bn_eps, int ridx,
                              int f, int R, int Tmax, void *workspace, hipStream_t s);
hipError_t launch_encoder_run_rows(const float *x, int T, const int *row_frames, const int *reset, float *out,
                                   const rnntPrednetBlock *blocks, int L, int F, float bn_eps, int ridx, int f, int R, int Tmax,
                                   void *workspace, hipStream_t s);
// lstm_train_kernels.hip (one LSTM layer for training: forward with saved activations, BPTT)
bool lstm_train_layout_ok(int R, int T, int H, int P, bool proj, size_t *bytes);
hipError_t launch_lstm_train_fwd(float *gates, const float *W_hh, const float *W_hr, float *y, float *c, float *h, int R, int T, int H,
                                 int P, void *workspace, hipStream_t s);
hipError_t launch_lstm_train_bwd(float *gates, const float *c, const float *dy, const float *W_hh, const float *W_hr, float *dr, int R,
                                 int T, int H, int P, void *workspace, hipStream_t s);
// frontend_kernels.hip (the streaming log-mel front end)
bool frontend_layout_ok(int K, int S, int L, int step, int M, int stack, int rm, size_t *bytes, int *max_rows);
hipError_t launch_frontend_begin(const float *window, const float *mel_weights, int K, int S, int L, int step, int M, int stack,
                                 int rm, void *workspace, hipStream_t s);
hipError_t launch_frontend_feed(const float *audio, int cs, const int *samples, const int *reset, const int *final_, int norm,
                                float *rows, int *counts, int K, int S, int L, int step, int M, int stack, int rm, void *workspace,
                                hipStream_t s);
}  // namespace rnnt

extern "C" {

int get_warprnnt_version(void) { return 1; }

const char *rnntGetStatusString(rnntStatus_t status) {
    switch (status) {
        case RNNT_STATUS_SUCCESS: return "no error";
        case RNNT_STATUS_MEMOPS_FAILED: return "hip memcpy or memset failed";
        case RNNT_STATUS_INVALID_VALUE: return "invalid value";
        case RNNT_STATUS_EXECUTION_FAILED: return "execution failed";
        case RNNT_STATUS_UNKNOWN_ERROR:
        default: return "unknown error";
    }
}

rnntStatus_t get_workspace_size(int maxT, int maxU, int minibatch, bool gpu, size_t *size_bytes) {
    if (!size_bytes || maxT <= 0 || maxU <= 0 || minibatch <= 0 || !gpu) return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = make_layout(maxT, maxU, minibatch).total;
    return RNNT_STATUS_SUCCESS;
}

// fill + lsm + sweeps on the caller's stream (stream order is the only dependency between the stages)
static rnntStatus_t run_forward(LossParams &p, const WsLayout &w, hipStream_t s) {
    if (lin_path_ok(p)) {  // small vocabulary, <= 256 lattice columns: the linear-domain lattice (rnnt_lin.h)
        hipError_t e = launch_lsm_lin(p, s);
        if (e != hipSuccess) return from_hip(e);
        return from_hip(launch_sweeps_lin(p, s));
    }
    // the patch kernels write the log-zero part of W themselves; the wave-per-cell kernels (large or unaligned vocabularies)
    // rely on a pre-filled W
    if (!tile_path_ok(p, false) && launch_fill(p.W, kFillByte, w.A - w.W, s) != hipSuccess) return RNNT_STATUS_MEMOPS_FAILED;
    p.precise = 1;  // the op's contract is 1e-4 on every input: float64 recurrence (the fused joints keep the float32 one up to 6 columns per lane)
    hipError_t e = launch_lsm(p, s);
    if (e != hipSuccess) return from_hip(e);
    return from_hip(launch_sweeps(p, s));
}

static rnntStatus_t validate(const void *acts, const void *labels, const void *ll, const void *il, const void *ws,
                      int V, int B, const rnntOptions &o) {
    if (!acts || !labels || !ll || !il || !ws) return RNNT_STATUS_INVALID_VALUE;
    if (V <= 0 || B <= 0) return RNNT_STATUS_INVALID_VALUE;
    rnntStatus_t st = check_options(o);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (o.blank_label >= V) return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

// Build-only split of compute_rnnt_loss so that an autograd caller can delay the gradient pass
// until the upstream gradient (run_rnnt.py:278: 1/global_batch) is known, and fold it in for free.
rnntStatus_t compute_rnnt_loss_fwd(const float *acts, const int *flat_labels, const int *label_lengths,
                                   const int *input_lengths, int alphabet_size, int minibatch, float *costs,
                                   void *workspace, rnntOptions options) {
    if (!costs) return RNNT_STATUS_INVALID_VALUE;
    rnntStatus_t st = validate(acts, flat_labels, label_lengths, input_lengths, workspace, alphabet_size, minibatch,
                               options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    LossParams p;
    if (!fill_loss_params(p, acts, nullptr, flat_labels, label_lengths, input_lengths, nullptr, alphabet_size, minibatch, costs,
                          workspace, options.maxT, options.maxU, options.blank_label))
        return RNNT_STATUS_INVALID_VALUE;
    hipStream_t s = (hipStream_t)options.stream;
    const WsLayout w = make_layout(options.maxT, options.maxU, minibatch);
    st = run_forward(p, w, s);
    if (st != RNNT_STATUS_SUCCESS || !lin_path_ok(p)) return st;
    return from_hip(launch_redo_lin(p, false, s));  // utterances the linear lattice handed back: log-domain sweeps (costs)
}

// The gradient pass.  On the linear path it ends with the hand-back launch (rnnt_lin_kernels.hip); a gradient buffer the
// patch kernels cannot write (not 16-byte aligned) sends every utterance through that launch.
static rnntStatus_t run_backward(LossParams &p, hipStream_t s) {
    if (!lin_path_ok(p)) return from_hip(launch_grad(p, s));
    const bool patch = tile_path_ok(p, true);
    if (patch) {
        hipError_t e = launch_grad_lin(p, s);
        if (e != hipSuccess) return from_hip(e);
    }
    return from_hip(launch_redo_lin(p, !patch, s));
}

rnntStatus_t compute_rnnt_loss_bwd(const float *acts, float *grads, const int *flat_labels,
                                   const int *label_lengths, const int *input_lengths, const float *cost_scale,
                                   int alphabet_size, int minibatch, void *workspace, rnntOptions options) {
    if (!grads) return RNNT_STATUS_INVALID_VALUE;
    rnntStatus_t st = validate(acts, flat_labels, label_lengths, input_lengths, workspace, alphabet_size, minibatch,
                               options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    LossParams p;
    if (!fill_loss_params(p, acts, grads, flat_labels, label_lengths, input_lengths, cost_scale, alphabet_size, minibatch, nullptr,
                          workspace, options.maxT, options.maxU, options.blank_label))
        return RNNT_STATUS_INVALID_VALUE;
    return run_backward(p, (hipStream_t)options.stream);
}

// compute_rnnt_loss with the upstream gradient folded in (cost_scale NULL = 1) and the build-only flags (include/rnnt.h):
// costs == NULL = the gradient pass alone (compute_rnnt_loss_bwd), grads == NULL = the forward alone.
// FastEmit's weight (include/rnnt.h): finite and in [0, 1] (a NaN fails both comparisons)
static bool fastemit_ok(float lambda) { return lambda >= 0.f && lambda <= 1.f; }

static rnntStatus_t loss_flags_call(const float *acts, float *grads, const int *flat_labels,
                                    const int *label_lengths, const int *input_lengths, const float *cost_scale,
                                    int alphabet_size, int minibatch, float *costs, void *workspace,
                                    const rnntOptions &options, unsigned int flags, float fastemit_lambda) {
    if (flags & ~(unsigned)RNNT_VISIT_ALL) return RNNT_STATUS_INVALID_VALUE;
    if (!grads)
        return compute_rnnt_loss_fwd(acts, flat_labels, label_lengths, input_lengths, alphabet_size, minibatch,
                                     costs, workspace, options);
    rnntStatus_t st = validate(acts, flat_labels, label_lengths, input_lengths, workspace, alphabet_size, minibatch,
                               options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    LossParams p;
    if (!fill_loss_params(p, acts, grads, flat_labels, label_lengths, input_lengths, cost_scale, alphabet_size, minibatch, costs,
                          workspace, options.maxT, options.maxU, options.blank_label))
        return RNNT_STATUS_INVALID_VALUE;
    p.visit_all = (flags & RNNT_VISIT_ALL) ? 1 : 0;
    p.fe_lambda = fastemit_lambda;  // (0: the plain gradient kernels)
    hipStream_t s = (hipStream_t)options.stream;
    if (costs) {
        const WsLayout w = make_layout(options.maxT, options.maxU, minibatch);
        st = run_forward(p, w, s);
        if (st != RNNT_STATUS_SUCCESS) return st;
    }
    return run_backward(p, s);
}

rnntStatus_t compute_rnnt_loss_flags(const float *acts, float *grads, const int *flat_labels,
                                     const int *label_lengths, const int *input_lengths, const float *cost_scale,
                                     int alphabet_size, int minibatch, float *costs, void *workspace,
                                     rnntOptions options, unsigned int flags) {
    return loss_flags_call(acts, grads, flat_labels, label_lengths, input_lengths, cost_scale, alphabet_size, minibatch, costs,
                           workspace, options, flags, 0.f);
}

// compute_rnnt_loss_flags with FastEmit regularisation of the gradients (include/rnnt.h); the costs do not depend on lambda
rnntStatus_t compute_rnnt_loss_fastemit(const float *acts, float *grads, const int *flat_labels,
                                        const int *label_lengths, const int *input_lengths, const float *cost_scale,
                                        int alphabet_size, int minibatch, float *costs, void *workspace,
                                        rnntOptions options, unsigned int flags, float fastemit_lambda) {
    if (!fastemit_ok(fastemit_lambda)) return RNNT_STATUS_INVALID_VALUE;
    return loss_flags_call(acts, grads, flat_labels, label_lengths, input_lengths, cost_scale, alphabet_size, minibatch, costs,
                           workspace, options, flags, fastemit_lambda);
}

rnntStatus_t compute_rnnt_loss_ex(const float *acts, float *grads, const int *flat_labels,
                                  const int *label_lengths, const int *input_lengths, const float *cost_scale,
                                  int alphabet_size, int minibatch, float *costs, void *workspace,
                                  rnntOptions options) {
    if (grads && !costs) return RNNT_STATUS_INVALID_VALUE;
    return compute_rnnt_loss_flags(acts, grads, flat_labels, label_lengths, input_lengths, cost_scale, alphabet_size, minibatch,
                                   costs, workspace, options, 0u);
}

rnntStatus_t compute_rnnt_loss(const float *acts, float *grads, const int *flat_labels,
                               const int *label_lengths, const int *input_lengths, int alphabet_size,
                               int minibatch, float *costs, void *workspace, rnntOptions options) {
    return compute_rnnt_loss_ex(acts, grads, flat_labels, label_lengths, input_lengths, nullptr, alphabet_size,
                                minibatch, costs, workspace, options);
}

rnntStatus_t get_joint_workspace_size(int maxT, int maxU, int minibatch, int joint_size, int alphabet_size,
                                      size_t *size_bytes) {
    if (!size_bytes || maxT <= 0 || maxU <= 0 || minibatch <= 0 || joint_size <= 0 || alphabet_size <= 0)
        return RNNT_STATUS_INVALID_VALUE;
    return from_hip(joint_workspace_bytes(maxT, maxU, minibatch, joint_size, alphabet_size, -1, size_bytes));
}

static rnntStatus_t joint_call(const float *enc_proj, const float *pred_proj, const float *W2, const float *b2,
                               const int *flat_labels, const int *label_lengths, const int *input_lengths,
                               const float *cost_scale, int joint_size, int alphabet_size, int minibatch, float *costs,
                               float *d_enc_proj, float *d_pred_proj, float *dW2, float *db2, int joint_dtype,
                               int phases, void *workspace, const rnntOptions &options, float fastemit_lambda = 0.f) {
    if (!enc_proj || !pred_proj || !W2 || !b2 || !flat_labels || !label_lengths || !input_lengths || !workspace)
        return RNNT_STATUS_INVALID_VALUE;
    if ((phases & 1) && !costs) return RNNT_STATUS_INVALID_VALUE;
    if (joint_size <= 0 || alphabet_size <= 0 || minibatch <= 0) return RNNT_STATUS_INVALID_VALUE;
    rnntStatus_t st = check_options(options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (options.blank_label >= alphabet_size) return RNNT_STATUS_INVALID_VALUE;
    if (options.maxU > 1024) return RNNT_STATUS_INVALID_VALUE;  // the fused joint paths are built on the register-resident sweeps
    if (joint_dtype & ~(0xff | RNNT_VISIT_ALL)) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype & RNNT_VISIT_ALL) phases |= 8;  // (launch_joint_loss: no occupancy floor in the backward)
    joint_dtype &= 0xff;
    if (!joint_dtype_supported(joint_dtype, joint_size, alphabet_size)) return RNNT_STATUS_INVALID_VALUE;
    const bool any_grad = d_enc_proj || d_pred_proj || dW2 || db2;
    if (any_grad && !(d_enc_proj && d_pred_proj && dW2 && db2)) return RNNT_STATUS_INVALID_VALUE;
    if ((phases & 2) && !(phases & 1) && !any_grad) return RNNT_STATUS_INVALID_VALUE;
    return from_hip(launch_joint_loss(enc_proj, pred_proj, W2, b2, flat_labels, label_lengths, input_lengths,
                                      cost_scale, joint_size, alphabet_size, minibatch, options.maxT, options.maxU,
                                      options.blank_label, costs, d_enc_proj, d_pred_proj, dW2, db2, joint_dtype,
                                      phases, workspace, (hipStream_t)options.stream, nullptr, fastemit_lambda));
}

rnntStatus_t compute_rnnt_joint_loss(const float *enc_proj, const float *pred_proj, const float *W2,
                                     const float *b2, const int *flat_labels, const int *label_lengths,
                                     const int *input_lengths, const float *cost_scale, int joint_size,
                                     int alphabet_size, int minibatch, float *costs, float *d_enc_proj,
                                     float *d_pred_proj, float *dW2, float *db2, int joint_dtype, void *workspace,
                                     rnntOptions options) {
    return joint_call(enc_proj, pred_proj, W2, b2, flat_labels, label_lengths, input_lengths, cost_scale, joint_size,
                      alphabet_size, minibatch, costs, d_enc_proj, d_pred_proj, dW2, db2, joint_dtype, 3, workspace,
                      options);
}

rnntStatus_t compute_rnnt_joint_loss_fwd(const float *enc_proj, const float *pred_proj, const float *W2,
                                         const float *b2, const int *flat_labels, const int *label_lengths,
                                         const int *input_lengths, int joint_size, int alphabet_size, int minibatch,
                                         float *costs, int joint_dtype, void *workspace, rnntOptions options) {
    return joint_call(enc_proj, pred_proj, W2, b2, flat_labels, label_lengths, input_lengths, nullptr, joint_size,
                      alphabet_size, minibatch, costs, nullptr, nullptr, nullptr, nullptr, joint_dtype, 1 | 4, workspace,
                      options);  // bit 2: a backward-only call follows (the forward leaves what that call needs)
}

rnntStatus_t compute_rnnt_joint_loss_bwd(const float *enc_proj, const float *pred_proj, const float *W2,
                                         const float *b2, const int *flat_labels, const int *label_lengths,
                                         const int *input_lengths, const float *cost_scale, int joint_size,
                                         int alphabet_size, int minibatch, float *d_enc_proj, float *d_pred_proj,
                                         float *dW2, float *db2, int joint_dtype, void *workspace,
                                         rnntOptions options) {
    if (!d_enc_proj) return RNNT_STATUS_INVALID_VALUE;
    return joint_call(enc_proj, pred_proj, W2, b2, flat_labels, label_lengths, input_lengths, cost_scale, joint_size,
                      alphabet_size, minibatch, nullptr, d_enc_proj, d_pred_proj, dW2, db2, joint_dtype, 2, workspace,
                      options);
}

// compute_rnnt_joint_loss_bwd with FastEmit regularisation (include/rnnt.h): the same backward from FastEmit's dlogits
rnntStatus_t compute_rnnt_joint_loss_bwd_fastemit(const float *enc_proj, const float *pred_proj, const float *W2,
                                                  const float *b2, const int *flat_labels, const int *label_lengths,
                                                  const int *input_lengths, const float *cost_scale, int joint_size,
                                                  int alphabet_size, int minibatch, float *d_enc_proj, float *d_pred_proj,
                                                  float *dW2, float *db2, int joint_dtype, void *workspace,
                                                  rnntOptions options, float fastemit_lambda) {
    if (!d_enc_proj || !fastemit_ok(fastemit_lambda)) return RNNT_STATUS_INVALID_VALUE;
    return joint_call(enc_proj, pred_proj, W2, b2, flat_labels, label_lengths, input_lengths, cost_scale, joint_size,
                      alphabet_size, minibatch, nullptr, d_enc_proj, d_pred_proj, dW2, db2, joint_dtype, 2, workspace,
                      options, fastemit_lambda);
}

// ---- the whole joint network (first Dense layer included) fused with the loss ----
rnntStatus_t get_joint_net_workspace_size(int maxT, int maxU, int minibatch, int hidden_size, int joint_size, int alphabet_size,
                                          size_t *size_bytes) {
    if (!size_bytes || maxT <= 0 || maxU <= 0 || minibatch <= 0 || hidden_size <= 0 || joint_size <= 0 || alphabet_size <= 0)
        return RNNT_STATUS_INVALID_VALUE;
    size_t base = 0;
    hipError_t e = joint_workspace_bytes(maxT, maxU, minibatch, joint_size, alphabet_size, -1, &base);
    if (e != hipSuccess) return from_hip(e);
    return from_hip(dense_workspace_bytes(minibatch, maxT, maxU, hidden_size, joint_size, base, size_bytes));
}

static rnntStatus_t joint_net_call(const float *enc, const float *pred, const float *W1, const float *b1, const float *W2,
                                   const float *b2, const int *flat_labels, const int *label_lengths, const int *input_lengths,
                                   const float *cost_scale, int hidden_size, int joint_size, int alphabet_size, int minibatch,
                                   float *costs, float *d_enc, float *d_pred, float *dW1, float *db1, float *dW2, float *db2,
                                   int joint_dtype, int phases, void *workspace, const rnntOptions &options,
                                   float fastemit_lambda = 0.f) {
    if (!enc || !pred || !W1 || !b1 || !W2 || !b2 || !flat_labels || !label_lengths || !input_lengths || !workspace)
        return RNNT_STATUS_INVALID_VALUE;
    if ((phases & 1) && !costs) return RNNT_STATUS_INVALID_VALUE;
    if (hidden_size <= 0 || joint_size <= 0 || alphabet_size <= 0 || minibatch <= 0) return RNNT_STATUS_INVALID_VALUE;
    rnntStatus_t st = check_options(options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (options.blank_label >= alphabet_size || options.maxU > 1024) return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)workspace & 255) != 0 || !dense_supported(hidden_size, joint_size)) return RNNT_STATUS_INVALID_VALUE;
    const bool any_grad = d_enc || d_pred || dW1 || db1 || dW2 || db2;
    if (any_grad && !(d_enc && d_pred && dW1 && db1 && dW2 && db2)) return RNNT_STATUS_INVALID_VALUE;
    if (any_grad && ((((uintptr_t)dW1 | (uintptr_t)db1 | (uintptr_t)d_enc | (uintptr_t)d_pred) & 15) != 0)) return RNNT_STATUS_INVALID_VALUE;  // 16-byte stores
    if ((((uintptr_t)enc | (uintptr_t)pred | (uintptr_t)W1 | (uintptr_t)b1) & 15) != 0) return RNNT_STATUS_INVALID_VALUE;
    if ((phases & 2) && !(phases & 1) && !any_grad) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype & ~(0xff | RNNT_VISIT_ALL)) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype & RNNT_VISIT_ALL) phases |= 8;  // (launch_joint_loss: no occupancy floor in the backward)
    joint_dtype &= 0xff;
    if (!joint_dtype_supported(joint_dtype, joint_size, alphabet_size)) return RNNT_STATUS_INVALID_VALUE;  // before anything is enqueued
    const int B = minibatch, T = options.maxT, U = options.maxU;
    hipStream_t s = (hipStream_t)options.stream;
    size_t base = 0;
    hipError_t e = joint_workspace_bytes(T, U, B, joint_size, alphabet_size, -1, &base);
    if (e != hipSuccess) return from_hip(e);
    // What the dense layer does on the way for the fused joint (JointHooks): with the f32-grade joint, the forward GEMM's
    // epilogue writes the e^{2x} tables and the table-range flag (the prep kernel then only builds the W2 images), the
    // backward-only call reuses the forward's workspace state; the reductions that produce d enc_proj / d pred_proj leave
    // their per-block abs-max entries for the backward GEMMs' operand scales.
    JointHooks hooks;
    hooks.prep_mode = 0;
    hooks.prefilled = 0;
    dense_hook_pointers(workspace, B, T, U, hidden_size, joint_size, base, &hooks.dmax_enc, &hooks.dmax_pred);
    float *expE = nullptr, *expP = nullptr, *tflag = nullptr;
    if (joint_dtype == 0) {
        if ((e = joint_aux_pointers(workspace, T, U, B, joint_size, alphabet_size, &expE, &expP, &tflag)) != hipSuccess) return from_hip(e);
        hooks.prep_mode = (phases & 1) ? 1 : 2;
    }
    if (phases & 1) {
        if (tflag) {  // the joint's edge-array pre-fill and its flag words (the GEMM epilogue raises one of them) in ONE launch
            if (launch_joint_prefill(workspace, T, U, B, joint_size, alphabet_size, s) != hipSuccess) return RNNT_STATUS_MEMOPS_FAILED;
            hooks.prefilled = 1;
        }
        if ((e = launch_dense_fwd(enc, pred, W1, b1, B, T, U, hidden_size, joint_size, workspace, base, expE, expP, tflag, s)) != hipSuccess)
            return from_hip(e);
    }
    float *ep, *pp, *dep, *dpp;
    dense_proj_pointers(workspace, B, T, U, hidden_size, joint_size, base, &ep, &pp, &dep, &dpp);
    const bool bwd = (phases & 2) && any_grad;
    e = launch_joint_loss(ep, pp, W2, b2, flat_labels, label_lengths, input_lengths, cost_scale, joint_size, alphabet_size, B, T, U,
                          options.blank_label, costs, bwd ? dep : nullptr, bwd ? dpp : nullptr, bwd ? dW2 : nullptr,
                          bwd ? db2 : nullptr, joint_dtype, phases, workspace, s, &hooks, fastemit_lambda);
    if (e != hipSuccess || !bwd) return from_hip(e);
    return from_hip(launch_dense_bwd(B, T, U, hidden_size, joint_size, d_enc, d_pred, dW1, db1, workspace, base, s));
}

rnntStatus_t compute_rnnt_joint_net_loss(const float *enc, const float *pred, const float *W1, const float *b1, const float *W2,
                                         const float *b2, const int *flat_labels, const int *label_lengths,
                                         const int *input_lengths, const float *cost_scale, int hidden_size, int joint_size,
                                         int alphabet_size, int minibatch, float *costs, float *d_enc, float *d_pred, float *dW1,
                                         float *db1, float *dW2, float *db2, int joint_dtype, void *workspace, rnntOptions options) {
    return joint_net_call(enc, pred, W1, b1, W2, b2, flat_labels, label_lengths, input_lengths, cost_scale, hidden_size, joint_size,
                          alphabet_size, minibatch, costs, d_enc, d_pred, dW1, db1, dW2, db2, joint_dtype, 3, workspace, options);
}

rnntStatus_t compute_rnnt_joint_net_loss_fwd(const float *enc, const float *pred, const float *W1, const float *b1, const float *W2,
                                             const float *b2, const int *flat_labels, const int *label_lengths,
                                             const int *input_lengths, int hidden_size, int joint_size, int alphabet_size,
                                             int minibatch, float *costs, int joint_dtype, void *workspace, rnntOptions options) {
    return joint_net_call(enc, pred, W1, b1, W2, b2, flat_labels, label_lengths, input_lengths, nullptr, hidden_size, joint_size,
                          alphabet_size, minibatch, costs, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, joint_dtype, 1 | 4,
                          workspace, options);
}

rnntStatus_t compute_rnnt_joint_net_loss_bwd(const float *enc, const float *pred, const float *W1, const float *b1, const float *W2,
                                             const float *b2, const int *flat_labels, const int *label_lengths,
                                             const int *input_lengths, const float *cost_scale, int hidden_size, int joint_size,
                                             int alphabet_size, int minibatch, float *d_enc, float *d_pred, float *dW1, float *db1,
                                             float *dW2, float *db2, int joint_dtype, void *workspace, rnntOptions options) {
    if (!d_enc) return RNNT_STATUS_INVALID_VALUE;
    return joint_net_call(enc, pred, W1, b1, W2, b2, flat_labels, label_lengths, input_lengths, cost_scale, hidden_size, joint_size,
                          alphabet_size, minibatch, nullptr, d_enc, d_pred, dW1, db1, dW2, db2, joint_dtype, 2, workspace, options);
}

rnntStatus_t compute_rnnt_joint_net_loss_bwd_fastemit(const float *enc, const float *pred, const float *W1, const float *b1,
                                                      const float *W2, const float *b2, const int *flat_labels,
                                                      const int *label_lengths, const int *input_lengths,
                                                      const float *cost_scale, int hidden_size, int joint_size,
                                                      int alphabet_size, int minibatch, float *d_enc, float *d_pred, float *dW1,
                                                      float *db1, float *dW2, float *db2, int joint_dtype, void *workspace,
                                                      rnntOptions options, float fastemit_lambda) {
    if (!d_enc || !fastemit_ok(fastemit_lambda)) return RNNT_STATUS_INVALID_VALUE;
    return joint_net_call(enc, pred, W1, b1, W2, b2, flat_labels, label_lengths, input_lengths, cost_scale, hidden_size, joint_size,
                          alphabet_size, minibatch, nullptr, d_enc, d_pred, dW1, db1, dW2, db2, joint_dtype, 2, workspace, options,
                          fastemit_lambda);
}

// The joint alone, for decoding (utils/decoding.py:6-18 evaluates dense_1 / dense_2 on one lattice cell per step).
rnntStatus_t compute_rnnt_joint_logits(const float *enc_proj, const float *pred_proj, const float *W2, const float *b2,
                                       int joint_size, int alphabet_size, int minibatch, float *logits, int joint_dtype,
                                       void *workspace, rnntOptions options) {
    if (!enc_proj || !pred_proj || !W2 || !b2 || !logits || !workspace) return RNNT_STATUS_INVALID_VALUE;
    if (joint_size <= 0 || alphabet_size <= 0 || minibatch <= 0) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype != 0 && joint_dtype != 1) return RNNT_STATUS_INVALID_VALUE;
    rnntStatus_t st = check_options(options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (options.maxU > 1024) return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    if (!joint_dtype_supported(joint_dtype, joint_size, alphabet_size)) return RNNT_STATUS_INVALID_VALUE;
    hipStream_t s = (hipStream_t)options.stream;
    if (joint_dtype == 1)
        return from_hip(launch_joint_logits_f16(enc_proj, pred_proj, W2, b2, joint_size, alphabet_size, minibatch, options.maxT,
                                                options.maxU, logits, workspace, s));
    return from_hip(launch_joint_logits(enc_proj, pred_proj, W2, b2, joint_size, alphabet_size, minibatch, options.maxT,
                                        options.maxU, logits, workspace, s));
}

// Rows (x u-tiles) the last f32-grade backward on this workspace visited / rows inside the utterances (include/rnnt.h).
rnntStatus_t get_rnnt_joint_backward_rows(void *workspace, int joint_size, int alphabet_size, int minibatch, rnntOptions options,
                                          int rows[2]) {
    if (!workspace || !rows || joint_size <= 0 || alphabet_size <= 0 || minibatch <= 0) return RNNT_STATUS_INVALID_VALUE;
    rnntStatus_t st = check_options(options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    const bool t32 = joint_dtype_supported(0, joint_size, alphabet_size), t16 = joint_dtype_supported(1, joint_size, alphabet_size);
    if (!t32 && !t16) return RNNT_STATUS_INVALID_VALUE;
    rows[0] = rows[1] = -1;
    rnntStatus_t r = RNNT_STATUS_SUCCESS;
    if (t32)
        r = from_hip(joint_backward_rows(workspace, options.maxT, options.maxU, minibatch, joint_size, alphabet_size, rows,
                                         (hipStream_t)options.stream));
    // (a shape both arithmetic types take, alphabet_size 128: whichever backward stamped the workspace last answers)
    if (r == RNNT_STATUS_SUCCESS && rows[1] < 0 && t16)
        r = from_hip(joint_f16_backward_rows(workspace, options.maxT, options.maxU, minibatch, joint_size, alphabet_size, rows,
                                             (hipStream_t)options.stream));
    return r;
}

// The whole joint network without the loss: first Dense layer (the library's split-precision GEMMs, as in the fused loss) + the
// joint, logits [minibatch, maxT, maxU, alphabet_size] out.  Workspace: get_joint_net_workspace_size().
rnntStatus_t compute_rnnt_joint_net_logits(const float *enc, const float *pred, const float *W1, const float *b1, const float *W2,
                                           const float *b2, int hidden_size, int joint_size, int alphabet_size, int minibatch,
                                           float *logits, int joint_dtype, void *workspace, rnntOptions options) {
    if (!enc || !pred || !W1 || !b1 || !W2 || !b2 || !logits || !workspace) return RNNT_STATUS_INVALID_VALUE;
    if (hidden_size <= 0 || joint_size <= 0 || alphabet_size <= 0 || minibatch <= 0) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype != 0 && joint_dtype != 1) return RNNT_STATUS_INVALID_VALUE;
    rnntStatus_t st = check_options(options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (options.maxU > 1024) return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)workspace & 255) != 0 || !dense_supported(hidden_size, joint_size)) return RNNT_STATUS_INVALID_VALUE;
    if ((((uintptr_t)enc | (uintptr_t)pred | (uintptr_t)W1 | (uintptr_t)b1) & 15) != 0) return RNNT_STATUS_INVALID_VALUE;
    if (!joint_dtype_supported(joint_dtype, joint_size, alphabet_size)) return RNNT_STATUS_INVALID_VALUE;  // before the GEMM is enqueued
    const int B = minibatch, T = options.maxT, U = options.maxU;
    hipStream_t s = (hipStream_t)options.stream;
    size_t base = 0;
    hipError_t e = joint_workspace_bytes(T, U, B, joint_size, alphabet_size, -1, &base);
    if (e != hipSuccess) return from_hip(e);
    // (the joint's own prep kernel builds the tanh tables here: one cell per call is the common case, nothing to save)
    if ((e = launch_dense_fwd(enc, pred, W1, b1, B, T, U, hidden_size, joint_size, workspace, base, nullptr, nullptr, nullptr, s)) != hipSuccess)
        return from_hip(e);
    float *ep, *pp, *dep, *dpp;
    dense_proj_pointers(workspace, B, T, U, hidden_size, joint_size, base, &ep, &pp, &dep, &dpp);
    if (joint_dtype == 1)
        return from_hip(launch_joint_logits_f16(ep, pp, W2, b2, joint_size, alphabet_size, B, T, U, logits, workspace, s));
    return from_hip(launch_joint_logits(ep, pp, W2, b2, joint_size, alphabet_size, B, T, U, logits, workspace, s));
}


// Batched greedy decoding (include/rnnt.h).  Everything is checked before anything is enqueued (rnnt_decode_host.h: check_greedy).
rnntStatus_t get_rnnt_greedy_workspace_size(int maxT, int minibatch, int joint_size, int alphabet_size, int joint_dtype,
                                            size_t *size_bytes) {
    if (!size_bytes) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype != 0 && joint_dtype != 1) return RNNT_STATUS_INVALID_VALUE;
    return greedy_workspace_bytes(maxT, minibatch, joint_size, alphabet_size, joint_dtype, size_bytes) == hipSuccess
               ? RNNT_STATUS_SUCCESS
               : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t compute_rnnt_greedy_begin(const float *enc_proj, const int *frame_lengths, const int *max_symbols, const float *W2,
                                       const float *b2, int joint_size, int alphabet_size, int minibatch, int max_per_frame,
                                       int joint_dtype, void *workspace, rnntOptions options) {
    if (!enc_proj || !frame_lengths || !W2 || !b2 || !workspace) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_greedy(options.maxT, joint_size, alphabet_size, minibatch, joint_dtype, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    return from_hip(launch_greedy_begin(enc_proj, frame_lengths, max_symbols, W2, b2, joint_size, alphabet_size, minibatch,
                                        options.maxT, max_per_frame, joint_dtype, workspace, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_greedy_step(const float *pred_proj, int *hyps, int max_hyp_len, int *hyp_lengths, float *scores,
                                      int *emitted, int *all_done, float *logit_stats, int joint_size, int alphabet_size,
                                      int minibatch, int joint_dtype, void *workspace, rnntOptions options) {
    if (!pred_proj || !hyps || !hyp_lengths || !scores || !emitted || !all_done || !workspace) return RNNT_STATUS_INVALID_VALUE;
    if (max_hyp_len <= 0 || (long long)max_hyp_len * minibatch >= (1ll << 31)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_greedy(options.maxT, joint_size, alphabet_size, minibatch, joint_dtype, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    return from_hip(launch_greedy_step(pred_proj, hyps, max_hyp_len, hyp_lengths, scores, emitted, all_done, logit_stats, nullptr,
                                       nullptr, nullptr, joint_size, alphabet_size, minibatch, options.maxT, options.blank_label,
                                       joint_dtype, workspace, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_greedy_step_timed(const float *pred_proj, int *hyps, int *hyp_frames, float *hyp_logp, int max_hyp_len,
                                            int *hyp_lengths, float *scores, int *emitted, int *all_done, float *logit_stats,
                                            const int *frame_base, int joint_size, int alphabet_size, int minibatch, int joint_dtype,
                                            void *workspace, rnntOptions options) {
    if (!pred_proj || !hyps || !hyp_frames || !hyp_logp || !hyp_lengths || !scores || !emitted || !all_done || !workspace)
        return RNNT_STATUS_INVALID_VALUE;
    if ((((uintptr_t)hyps | (uintptr_t)hyp_frames | (uintptr_t)hyp_logp | (uintptr_t)frame_base) & 3) != 0)
        return RNNT_STATUS_INVALID_VALUE;
    if (max_hyp_len <= 0 || (long long)max_hyp_len * minibatch >= (1ll << 31)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_greedy(options.maxT, joint_size, alphabet_size, minibatch, joint_dtype, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    return from_hip(launch_greedy_step(pred_proj, hyps, max_hyp_len, hyp_lengths, scores, emitted, all_done, logit_stats, hyp_frames,
                                       hyp_logp, frame_base, joint_size, alphabet_size, minibatch, options.maxT, options.blank_label,
                                       joint_dtype, workspace, (hipStream_t)options.stream));
}


// Batched beam search (include/rnnt.h).  Everything is checked before anything is enqueued (rnnt_decode_host.h: check_beam).
// Kept as it was: the untimed begin, step and results check no alignment, their timed twins further down do.
rnntStatus_t get_rnnt_beam_workspace_size(int maxT, int minibatch, int beam, int joint_size, int alphabet_size, int joint_dtype,
                                          size_t *size_bytes) {
    if (!size_bytes) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype != 0 && joint_dtype != 1) return RNNT_STATUS_INVALID_VALUE;
    return beam_workspace_bytes(maxT, minibatch, beam, joint_size, alphabet_size, joint_dtype, false, size_bytes) == hipSuccess
               ? RNNT_STATUS_SUCCESS
               : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t compute_rnnt_beam_begin(const float *enc_proj, const int *frame_lengths, const float *W2, const float *b2,
                                     int joint_size, int alphabet_size, int minibatch, int beam, int joint_dtype, void *workspace,
                                     rnntOptions options) {
    if (!enc_proj || !frame_lengths || !W2 || !b2) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st =
        check_beam(options.maxT, joint_size, alphabet_size, minibatch, beam, joint_dtype, workspace, options, false);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_beam_begin(enc_proj, frame_lengths, W2, b2, joint_size, alphabet_size, minibatch, options.maxT, beam,
                                      joint_dtype, false, workspace, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_beam_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits, int *topk_symbols,
                                    float *lse, int joint_size, int alphabet_size, int minibatch, int beam, int joint_dtype,
                                    void *workspace, rnntOptions options) {
    return beam_step_call(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, joint_size, alphabet_size, minibatch, beam,
                          joint_dtype, workspace, options, false);
}

rnntStatus_t compute_rnnt_beam_results(int *hyps, int *hyp_lengths, float *scores, int joint_size, int alphabet_size, int minibatch,
                                       int beam, int joint_dtype, void *workspace, rnntOptions options) {
    if (!hyps || !hyp_lengths || !scores) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st =
        check_beam(options.maxT, joint_size, alphabet_size, minibatch, beam, joint_dtype, workspace, options, false);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_beam_results(hyps, hyp_lengths, scores, nullptr, nullptr, nullptr, nullptr, joint_size, alphabet_size,
                                        minibatch, options.maxT, beam, options.maxT, joint_dtype, workspace,
                                        (hipStream_t)options.stream));
}


// The prediction-network step (include/rnnt.h).  Everything is checked before anything is enqueued.
static rnntStatus_t check_prednet(const rnntPrednetBlock *blocks, int num_blocks, int embed_size, int vocab_size, int joint_size,
                                  int rows, const void *workspace, bool weights, const rnntOptions &o) {
    if (!blocks || !workspace) return RNNT_STATUS_INVALID_VALUE;
    if (o.loc != RNNT_GPU) return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    if (!prednet_layout_ok(blocks, num_blocks, embed_size, vocab_size, joint_size, rows, nullptr)) return RNNT_STATUS_INVALID_VALUE;
    if (weights) {
        for (int l = 0; l < num_blocks; ++l) {
            const rnntPrednetBlock &b = blocks[l];
            if (!b.W_ih || !b.W_hh || !b.b_ih || !b.b_hh || !b.ln_weight || !b.ln_bias) return RNNT_STATUS_INVALID_VALUE;
            if (!aligned16(b.W_ih) || !aligned16(b.W_hh) || !aligned16(b.b_ih) || !aligned16(b.b_hh) || !aligned16(b.W_hr) ||
                !aligned16(b.ln_weight) || !aligned16(b.ln_bias))
                return RNNT_STATUS_INVALID_VALUE;
        }
    }
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t get_rnnt_prednet_workspace_size(const rnntPrednetBlock *blocks, int num_blocks, int embed_size, int vocab_size,
                                             int joint_size, int rows, size_t *size_bytes) {
    if (!size_bytes) return RNNT_STATUS_INVALID_VALUE;
    return prednet_layout_ok(blocks, num_blocks, embed_size, vocab_size, joint_size, rows, size_bytes) ? RNNT_STATUS_SUCCESS
                                                                                                       : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t compute_rnnt_prednet_begin(const float *embedding, const rnntPrednetBlock *blocks, int num_blocks, int embed_size,
                                        int vocab_size, const float *W1, int joint_size, int rows, float *pred_proj_out,
                                        void *workspace, rnntOptions options) {
    if (!embedding || !W1 || !pred_proj_out) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned16(embedding) || !aligned16(W1) || !aligned16(pred_proj_out)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_prednet(blocks, num_blocks, embed_size, vocab_size, joint_size, rows, workspace, true, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_prednet_begin(embedding, blocks, num_blocks, embed_size, vocab_size, W1, joint_size, rows, pred_proj_out,
                                         workspace, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_prednet_step(const int *emitted, const int *parents, float *pred_proj_out, const rnntPrednetBlock *blocks,
                                       int num_blocks, int embed_size, int vocab_size, int joint_size, int rows, void *workspace,
                                       rnntOptions options) {
    if (!emitted || !pred_proj_out) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned16(emitted) || !aligned16(parents) || !aligned16(pred_proj_out)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_prednet(blocks, num_blocks, embed_size, vocab_size, joint_size, rows, workspace, false, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_prednet_step(emitted, parents, pred_proj_out, blocks, num_blocks, embed_size, vocab_size, joint_size, rows,
                                        workspace, (hipStream_t)options.stream));
}


// The encoder (include/rnnt.h).  Everything is checked before anything is enqueued.
static rnntStatus_t check_encoder(const rnntPrednetBlock *blocks, int num_layers, int feat_size, float bn_eps, int reduction_index,
                                  int reduction_factor, int rows, int max_frames, const void *workspace, bool weights,
                                  const rnntOptions &o) {
    if (!blocks || !workspace) return RNNT_STATUS_INVALID_VALUE;
    if (o.loc != RNNT_GPU) return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    if (!encoder_layout_ok(blocks, num_layers, feat_size, bn_eps, reduction_index, reduction_factor, rows, max_frames, nullptr))
        return RNNT_STATUS_INVALID_VALUE;
    if (weights) {
        for (int l = 0; l < num_layers; ++l) {
            const rnntPrednetBlock &b = blocks[l];
            if (!b.W_ih || !b.W_hh || !b.b_ih || !b.b_hh || !b.ln_weight || !b.ln_bias) return RNNT_STATUS_INVALID_VALUE;
            if (!aligned16(b.W_ih) || !aligned16(b.W_hh) || !aligned16(b.b_ih) || !aligned16(b.b_hh) || !aligned16(b.W_hr) ||
                !aligned16(b.ln_weight) || !aligned16(b.ln_bias))
                return RNNT_STATUS_INVALID_VALUE;
        }
    }
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t get_rnnt_encoder_workspace_size(const rnntPrednetBlock *blocks, int num_layers, int feat_size, int reduction_index,
                                             int reduction_factor, int rows, int max_frames, size_t *size_bytes) {
    if (!size_bytes) return RNNT_STATUS_INVALID_VALUE;
    return encoder_layout_ok(blocks, num_layers, feat_size, 0.f, reduction_index, reduction_factor, rows, max_frames, size_bytes)
               ? RNNT_STATUS_SUCCESS
               : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t compute_rnnt_encoder_begin(const rnntPrednetBlock *blocks, int num_layers, int feat_size, const float *bn_mean,
                                        const float *bn_var, const float *bn_weight, const float *bn_bias, float bn_eps,
                                        int reduction_index, int reduction_factor, int rows, int max_frames, void *workspace,
                                        rnntOptions options) {
    if (!bn_mean || !bn_var || !bn_weight || !bn_bias) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned16(bn_mean) || !aligned16(bn_var) || !aligned16(bn_weight) || !aligned16(bn_bias)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_encoder(blocks, num_layers, feat_size, bn_eps, reduction_index, reduction_factor, rows, max_frames,
                                          workspace, true, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_encoder_begin(blocks, num_layers, feat_size, bn_mean, bn_var, bn_weight, bn_bias, bn_eps, reduction_index,
                                         reduction_factor, rows, max_frames, workspace, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_encoder_run(const float *x, int frames, float *out, const rnntPrednetBlock *blocks, int num_layers,
                                      int feat_size, float bn_eps, int reduction_index, int reduction_factor, int rows, int max_frames,
                                      void *workspace, rnntOptions options) {
    if (!x || !out || !aligned16(x) || !aligned16(out)) return RNNT_STATUS_INVALID_VALUE;
    if (frames < 1 || frames > max_frames) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_encoder(blocks, num_layers, feat_size, bn_eps, reduction_index, reduction_factor, rows, max_frames,
                                          workspace, false, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_encoder_run(x, frames, out, blocks, num_layers, feat_size, bn_eps, reduction_index, reduction_factor, rows,
                                       max_frames, workspace, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_encoder_run_rows(const float *x, int frames, const int *row_frames, const int *reset, float *out,
                                           const rnntPrednetBlock *blocks, int num_layers, int feat_size, float bn_eps,
                                           int reduction_index, int reduction_factor, int rows, int max_frames, void *workspace,
                                           rnntOptions options) {
    if (!x || !out || !row_frames || !aligned16(x) || !aligned16(out)) return RNNT_STATUS_INVALID_VALUE;
    if (frames < 1 || frames > max_frames) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_encoder(blocks, num_layers, feat_size, bn_eps, reduction_index, reduction_factor, rows, max_frames,
                                          workspace, false, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_encoder_run_rows(x, frames, row_frames, reset, out, blocks, num_layers, feat_size, bn_eps, reduction_index,
                                            reduction_factor, rows, max_frames, workspace, (hipStream_t)options.stream));
}


// Streaming greedy decoding (include/rnnt.h).  Everything is checked before anything is enqueued.
rnntStatus_t compute_rnnt_prednet_reset(const int *reset, float *pred_proj_out, const rnntPrednetBlock *blocks, int num_blocks,
                                        int embed_size, int vocab_size, int joint_size, int rows, void *workspace, rnntOptions options) {
    if (!reset || !pred_proj_out || !aligned16(pred_proj_out)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_prednet(blocks, num_blocks, embed_size, vocab_size, joint_size, rows, workspace, false, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_prednet_reset(reset, pred_proj_out, blocks, num_blocks, embed_size, vocab_size, joint_size, rows, workspace,
                                         (hipStream_t)options.stream));
}

rnntStatus_t get_rnnt_greedy_stream_workspace_size(int max_chunk_frames, int slots, int enc_width, int joint_size, int alphabet_size,
                                                   int joint_dtype, size_t *size_bytes) {
    if (!size_bytes) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype != 0 && joint_dtype != 1) return RNNT_STATUS_INVALID_VALUE;
    return greedy_stream_workspace_bytes(max_chunk_frames, slots, enc_width, joint_size, alphabet_size, joint_dtype, size_bytes) ==
                   hipSuccess
               ? RNNT_STATUS_SUCCESS
               : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t compute_rnnt_greedy_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2, int enc_width,
                                              int joint_size, int alphabet_size, int slots, int joint_dtype, void *workspace,
                                              rnntOptions options) {
    if (!W1 || !b1 || !W2 || !b2) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st =
        check_greedy_stream(options.maxT, slots, enc_width, joint_size, alphabet_size, joint_dtype, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_greedy_stream_begin(W1, b1, W2, b2, enc_width, joint_size, alphabet_size, slots, options.maxT, joint_dtype,
                                               workspace, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_greedy_stream_feed(const float *enc, int enc_frames, const int *chunk_frames, const int *reset,
                                             const int *final_chunk, const int *max_symbols, int max_per_frame, int *hyp_lengths,
                                             float *scores, int *all_done, int enc_width, int joint_size, int alphabet_size, int slots,
                                             int joint_dtype, void *workspace, rnntOptions options) {
    if (!chunk_frames || !hyp_lengths || !scores || !all_done) return RNNT_STATUS_INVALID_VALUE;
    if (enc_frames < 0 || enc_frames > options.maxT || (enc_frames > 0 && !enc)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st =
        check_greedy_stream(options.maxT, slots, enc_width, joint_size, alphabet_size, joint_dtype, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_greedy_stream_feed(enc, enc_frames, chunk_frames, reset, final_chunk, max_symbols, max_per_frame,
                                              hyp_lengths, scores, all_done, nullptr, enc_width, joint_size, alphabet_size, slots,
                                              options.maxT, joint_dtype, workspace, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_greedy_stream_feed_timed(const float *enc, int enc_frames, const int *chunk_frames, const int *reset,
                                                   const int *final_chunk, const int *max_symbols, int max_per_frame,
                                                   int *hyp_lengths, float *scores, int *all_done, int *frame_base, int enc_width,
                                                   int joint_size, int alphabet_size, int slots, int joint_dtype, void *workspace,
                                                   rnntOptions options) {
    if (!chunk_frames || !hyp_lengths || !scores || !all_done || !frame_base || ((uintptr_t)frame_base & 3) != 0)
        return RNNT_STATUS_INVALID_VALUE;
    if (enc_frames < 0 || enc_frames > options.maxT || (enc_frames > 0 && !enc)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st =
        check_greedy_stream(options.maxT, slots, enc_width, joint_size, alphabet_size, joint_dtype, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_greedy_stream_feed(enc, enc_frames, chunk_frames, reset, final_chunk, max_symbols, max_per_frame,
                                              hyp_lengths, scores, all_done, frame_base, enc_width, joint_size, alphabet_size, slots,
                                              options.maxT, joint_dtype, workspace, (hipStream_t)options.stream));
}

// The beam stream (include/rnnt.h; rnnt_decode_host.h: check_beam_stream).  The timed entry points further down are the same
// bodies on the workspace layout that also holds the {frame, log-probability} rows.
rnntStatus_t get_rnnt_beam_stream_workspace_size(int max_chunk_frames, int slots, int beam, int max_hyp_len, int enc_width,
                                                 int joint_size, int alphabet_size, int joint_dtype, size_t *size_bytes) {
    if (!size_bytes) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype != 0 && joint_dtype != 1) return RNNT_STATUS_INVALID_VALUE;
    return beam_stream_workspace_bytes(max_chunk_frames, slots, beam, max_hyp_len, enc_width, joint_size, alphabet_size, joint_dtype,
                                       false, size_bytes) == hipSuccess
               ? RNNT_STATUS_SUCCESS
               : RNNT_STATUS_INVALID_VALUE;
}

static rnntStatus_t beam_stream_begin_call(const float *W1, const float *b1, const float *W2, const float *b2, int enc_width,
                                           int joint_size, int alphabet_size, int slots, int beam, int max_hyp_len, int joint_dtype,
                                           void *workspace, const rnntOptions &options, bool timed) {
    if (!W1 || !b1 || !W2 || !b2 || !aligned4(W1) || !aligned4(b1) || !aligned4(W2) || !aligned4(b2)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_beam_stream(options.maxT, slots, beam, max_hyp_len, enc_width, joint_size, alphabet_size, joint_dtype,
                                              workspace, options, timed);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_beam_stream_begin(W1, b1, W2, b2, enc_width, joint_size, alphabet_size, slots, options.maxT, beam,
                                             max_hyp_len, joint_dtype, timed, workspace, (hipStream_t)options.stream));
}

static rnntStatus_t beam_stream_feed_call(const float *enc, int enc_frames, const int *chunk_frames, const int *reset,
                                          const int *final_chunk, int enc_width, int joint_size, int alphabet_size, int slots,
                                          int beam, int max_hyp_len, int joint_dtype, void *workspace, const rnntOptions &options,
                                          bool timed) {
    if (!chunk_frames || !aligned4(enc) || !aligned4(chunk_frames) || !aligned4(reset) || !aligned4(final_chunk))
        return RNNT_STATUS_INVALID_VALUE;
    if (enc_frames < 0 || enc_frames > options.maxT || (enc_frames > 0 && !enc)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_beam_stream(options.maxT, slots, beam, max_hyp_len, enc_width, joint_size, alphabet_size, joint_dtype,
                                              workspace, options, timed);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_beam_stream_feed(enc, enc_frames, chunk_frames, reset, final_chunk, enc_width, joint_size, alphabet_size,
                                            slots, options.maxT, beam, max_hyp_len, joint_dtype, timed, workspace,
                                            (hipStream_t)options.stream));
}

// timed: hyp_frames and hyp_logp are required; untimed: the three timed outputs are NULL
static rnntStatus_t beam_stream_results_call(int *hyps, int *hyp_lengths, float *scores, int *stable_lengths, int *hyp_frames,
                                             float *hyp_logp, int *timed_stable_lengths, int joint_size, int alphabet_size, int slots,
                                             int beam, int max_hyp_len, int joint_dtype, void *workspace, const rnntOptions &options,
                                             bool timed) {
    if (!hyps || !hyp_lengths || !scores || (timed && (!hyp_frames || !hyp_logp))) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(hyps) || !aligned4(hyp_lengths) || !aligned4(scores) || !aligned4(stable_lengths) || !aligned4(hyp_frames) ||
        !aligned4(hyp_logp) || !aligned4(timed_stable_lengths))
        return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_beam_stream(options.maxT, slots, beam, max_hyp_len, 1, joint_size, alphabet_size, joint_dtype,
                                              workspace, options, timed);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_beam_results(hyps, hyp_lengths, scores, stable_lengths, hyp_frames, hyp_logp, timed_stable_lengths,
                                        joint_size, alphabet_size, slots, options.maxT, beam, max_hyp_len, joint_dtype, workspace,
                                        (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_beam_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2, int enc_width,
                                            int joint_size, int alphabet_size, int slots, int beam, int max_hyp_len, int joint_dtype,
                                            void *workspace, rnntOptions options) {
    return beam_stream_begin_call(W1, b1, W2, b2, enc_width, joint_size, alphabet_size, slots, beam, max_hyp_len, joint_dtype, workspace,
                                  options, false);
}

rnntStatus_t compute_rnnt_beam_stream_feed(const float *enc, int enc_frames, const int *chunk_frames, const int *reset,
                                           const int *final_chunk, int enc_width, int joint_size, int alphabet_size, int slots,
                                           int beam, int max_hyp_len, int joint_dtype, void *workspace, rnntOptions options) {
    return beam_stream_feed_call(enc, enc_frames, chunk_frames, reset, final_chunk, enc_width, joint_size, alphabet_size, slots, beam,
                                 max_hyp_len, joint_dtype, workspace, options, false);
}

rnntStatus_t compute_rnnt_beam_stream_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits, int *topk_symbols,
                                           float *lse, int joint_size, int alphabet_size, int slots, int beam, int max_hyp_len,
                                           int joint_dtype, void *workspace, rnntOptions options) {
    return beam_stream_step_call(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, joint_size, alphabet_size, slots, beam,
                                 max_hyp_len, joint_dtype, workspace, options, false);
}

rnntStatus_t compute_rnnt_beam_stream_results(int *hyps, int *hyp_lengths, float *scores, int *stable_lengths, int joint_size,
                                              int alphabet_size, int slots, int beam, int max_hyp_len, int joint_dtype,
                                              void *workspace, rnntOptions options) {
    return beam_stream_results_call(hyps, hyp_lengths, scores, stable_lengths, nullptr, nullptr, nullptr, joint_size, alphabet_size,
                                    slots, beam, max_hyp_len, joint_dtype, workspace, options, false);
}

// The timed beam searches (include/rnnt.h): the same checks and launches on the workspace layout that also holds the
// {frame, log-probability} rows.
rnntStatus_t get_rnnt_beam_timed_workspace_size(int maxT, int minibatch, int beam, int joint_size, int alphabet_size, int joint_dtype,
                                                size_t *size_bytes) {
    if (!size_bytes) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype != 0 && joint_dtype != 1) return RNNT_STATUS_INVALID_VALUE;
    return beam_workspace_bytes(maxT, minibatch, beam, joint_size, alphabet_size, joint_dtype, true, size_bytes) == hipSuccess
               ? RNNT_STATUS_SUCCESS
               : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t compute_rnnt_beam_timed_begin(const float *enc_proj, const int *frame_lengths, const float *W2, const float *b2,
                                           int joint_size, int alphabet_size, int minibatch, int beam, int joint_dtype,
                                           void *workspace, rnntOptions options) {
    if (!enc_proj || !frame_lengths || !W2 || !b2 || !aligned4(enc_proj) || !aligned4(frame_lengths) || !aligned4(W2) || !aligned4(b2))
        return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st =
        check_beam(options.maxT, joint_size, alphabet_size, minibatch, beam, joint_dtype, workspace, options, true);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_beam_begin(enc_proj, frame_lengths, W2, b2, joint_size, alphabet_size, minibatch, options.maxT, beam,
                                      joint_dtype, true, workspace, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_beam_timed_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits, int *topk_symbols,
                                          float *lse, int joint_size, int alphabet_size, int minibatch, int beam, int joint_dtype,
                                          void *workspace, rnntOptions options) {
    return beam_step_call(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, joint_size, alphabet_size, minibatch, beam,
                          joint_dtype, workspace, options, true);
}

rnntStatus_t compute_rnnt_beam_timed_results(int *hyps, int *hyp_lengths, float *scores, int *hyp_frames, float *hyp_logp,
                                             int joint_size, int alphabet_size, int minibatch, int beam, int joint_dtype,
                                             void *workspace, rnntOptions options) {
    if (!hyps || !hyp_lengths || !scores || !hyp_frames || !hyp_logp) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(hyps) || !aligned4(hyp_lengths) || !aligned4(scores) || !aligned4(hyp_frames) || !aligned4(hyp_logp))
        return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st =
        check_beam(options.maxT, joint_size, alphabet_size, minibatch, beam, joint_dtype, workspace, options, true);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_beam_results(hyps, hyp_lengths, scores, nullptr, hyp_frames, hyp_logp, nullptr, joint_size, alphabet_size,
                                        minibatch, options.maxT, beam, options.maxT, joint_dtype, workspace,
                                        (hipStream_t)options.stream));
}

rnntStatus_t get_rnnt_beam_stream_timed_workspace_size(int max_chunk_frames, int slots, int beam, int max_hyp_len, int enc_width,
                                                       int joint_size, int alphabet_size, int joint_dtype, size_t *size_bytes) {
    if (!size_bytes) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype != 0 && joint_dtype != 1) return RNNT_STATUS_INVALID_VALUE;
    return beam_stream_workspace_bytes(max_chunk_frames, slots, beam, max_hyp_len, enc_width, joint_size, alphabet_size, joint_dtype,
                                       true, size_bytes) == hipSuccess
               ? RNNT_STATUS_SUCCESS
               : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t compute_rnnt_beam_stream_timed_begin(const float *W1, const float *b1, const float *W2, const float *b2, int enc_width,
                                                  int joint_size, int alphabet_size, int slots, int beam, int max_hyp_len,
                                                  int joint_dtype, void *workspace, rnntOptions options) {
    return beam_stream_begin_call(W1, b1, W2, b2, enc_width, joint_size, alphabet_size, slots, beam, max_hyp_len, joint_dtype, workspace,
                                  options, true);
}

rnntStatus_t compute_rnnt_beam_stream_timed_feed(const float *enc, int enc_frames, const int *chunk_frames, const int *reset,
                                                 const int *final_chunk, int enc_width, int joint_size, int alphabet_size, int slots,
                                                 int beam, int max_hyp_len, int joint_dtype, void *workspace, rnntOptions options) {
    return beam_stream_feed_call(enc, enc_frames, chunk_frames, reset, final_chunk, enc_width, joint_size, alphabet_size, slots, beam,
                                 max_hyp_len, joint_dtype, workspace, options, true);
}

rnntStatus_t compute_rnnt_beam_stream_timed_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                                 int *topk_symbols, float *lse, int joint_size, int alphabet_size, int slots, int beam,
                                                 int max_hyp_len, int joint_dtype, void *workspace, rnntOptions options) {
    return beam_stream_step_call(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, joint_size, alphabet_size, slots, beam,
                                 max_hyp_len, joint_dtype, workspace, options, true);
}

rnntStatus_t compute_rnnt_beam_stream_timed_results(int *hyps, int *hyp_lengths, float *scores, int *stable_lengths, int *hyp_frames,
                                                    float *hyp_logp, int *timed_stable_lengths, int joint_size, int alphabet_size,
                                                    int slots, int beam, int max_hyp_len, int joint_dtype, void *workspace,
                                                    rnntOptions options) {
    return beam_stream_results_call(hyps, hyp_lengths, scores, stable_lengths, hyp_frames, hyp_logp, timed_stable_lengths, joint_size,
                                    alphabet_size, slots, beam, max_hyp_len, joint_dtype, workspace, options, true);
}

// The LSTM layer for training (include/rnnt.h).  Everything is checked before anything is enqueued.
static rnntStatus_t check_lstm_train(int rows, int frames, int hidden, int proj, const float *W_hh, const float *W_hr,
                                     const void *workspace, const rnntOptions &o) {
    if (!W_hh || !workspace || !aligned16(W_hh) || !aligned16(W_hr)) return RNNT_STATUS_INVALID_VALUE;
    if (o.loc != RNNT_GPU) return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    return lstm_train_layout_ok(rows, frames, hidden, proj, W_hr != nullptr, nullptr) ? RNNT_STATUS_SUCCESS : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t get_rnnt_lstm_train_workspace_size(int rows, int frames, int hidden, int proj, size_t *size_bytes) {
    if (!size_bytes) return RNNT_STATUS_INVALID_VALUE;
    return lstm_train_layout_ok(rows, frames, hidden, proj, proj < hidden, size_bytes) ? RNNT_STATUS_SUCCESS
                                                                                       : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t compute_rnnt_lstm_train_fwd(float *gates, const float *W_hh, const float *W_hr, float *y, float *c, float *h, int rows,
                                         int frames, int hidden, int proj, void *workspace, rnntOptions options) {
    if (!gates || !y || !c || (W_hr && !h)) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned16(gates) || !aligned16(y) || !aligned16(c) || !aligned16(h)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_lstm_train(rows, frames, hidden, proj, W_hh, W_hr, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_lstm_train_fwd(gates, W_hh, W_hr, y, c, h, rows, frames, hidden, proj, workspace,
                                          (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_lstm_train_bwd(float *gates, const float *c, const float *dy, const float *W_hh, const float *W_hr,
                                         float *dr, int rows, int frames, int hidden, int proj, void *workspace, rnntOptions options) {
    if (!gates || !c || !dy || (W_hr && !dr)) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned16(gates) || !aligned16(c) || !aligned16(dy) || !aligned16(dr)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_lstm_train(rows, frames, hidden, proj, W_hh, W_hr, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_lstm_train_bwd(gates, c, dy, W_hh, W_hr, dr, rows, frames, hidden, proj, workspace,
                                          (hipStream_t)options.stream));
}

// The streaming log-mel front end (include/rnnt.h).  Everything is checked before anything is enqueued.
static rnntStatus_t check_frontend(int max_chunk_samples, int slots, int frame_len, int frame_step, int mel_bins, int stack,
                                   int row_multiple, const void *workspace, const rnntOptions &o) {
    if (!workspace || ((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    if (o.loc != RNNT_GPU) return RNNT_STATUS_INVALID_VALUE;
    return frontend_layout_ok(max_chunk_samples, slots, frame_len, frame_step, mel_bins, stack, row_multiple, nullptr, nullptr)
               ? RNNT_STATUS_SUCCESS
               : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t get_rnnt_frontend_workspace_size(int max_chunk_samples, int slots, int frame_len, int frame_step, int mel_bins,
                                              int stack, int row_multiple, size_t *size_bytes) {
    if (!size_bytes) return RNNT_STATUS_INVALID_VALUE;
    return frontend_layout_ok(max_chunk_samples, slots, frame_len, frame_step, mel_bins, stack, row_multiple, size_bytes, nullptr)
               ? RNNT_STATUS_SUCCESS
               : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t compute_rnnt_frontend_begin(const float *window, const float *mel_weights, int max_chunk_samples, int slots,
                                         int frame_len, int frame_step, int mel_bins, int stack, int row_multiple, void *workspace,
                                         rnntOptions options) {
    if (!window || !mel_weights || !aligned4(window) || !aligned4(mel_weights)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st =
        check_frontend(max_chunk_samples, slots, frame_len, frame_step, mel_bins, stack, row_multiple, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_frontend_begin(window, mel_weights, max_chunk_samples, slots, frame_len, frame_step, mel_bins, stack,
                                          row_multiple, workspace, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_frontend_feed(const float *audio, int chunk_samples, const int *samples, const int *reset,
                                        const int *final_chunk, int norm, float *rows_out, int *row_counts, int max_chunk_samples,
                                        int slots, int frame_len, int frame_step, int mel_bins, int stack, int row_multiple,
                                        void *workspace, rnntOptions options) {
    if (!samples || !rows_out || !row_counts) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(audio) || !aligned4(samples) || !aligned4(reset) || !aligned4(final_chunk) || !aligned4(rows_out) ||
        !aligned4(row_counts))
        return RNNT_STATUS_INVALID_VALUE;
    if (chunk_samples < 0 || chunk_samples > max_chunk_samples || (chunk_samples > 0 && !audio)) return RNNT_STATUS_INVALID_VALUE;
    if (norm != 0 && norm != 1) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st =
        check_frontend(max_chunk_samples, slots, frame_len, frame_step, mel_bins, stack, row_multiple, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_frontend_feed(audio, chunk_samples, samples, reset, final_chunk, norm, rows_out, row_counts,
                                         max_chunk_samples, slots, frame_len, frame_step, mel_bins, stack, row_multiple, workspace,
                                         (hipStream_t)options.stream));
}

// Forced alignment (include/rnnt.h).  Everything is checked before anything is enqueued.
static rnntStatus_t check_align(const void *labels, const void *ll, const void *il, const void *ws, int V, int B,
                                const rnntOptions &o) {
    if (!labels || !ll || !il || !ws) return RNNT_STATUS_INVALID_VALUE;
    if (V < 2 || B <= 0) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_options(o);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (o.blank_label >= V) return RNNT_STATUS_INVALID_VALUE;
    const long long cells = (long long)B * o.maxT * o.maxU;
    if (cells >= (1ll << 31)) return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)ws & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(labels) || !aligned4(ll) || !aligned4(il)) return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

static void fill_align(AlignParams &p, const int *labels, const int *ll, const int *il, int V, int B, void *ws,
                       const rnntOptions &o) {
    const AlignLayout w = make_align_layout(o.maxT, o.maxU, B);
    p = AlignParams{};
    p.labels = labels, p.label_lengths = ll, p.input_lengths = il;
    p.cells = (float2 *)((char *)ws + w.cells);
    p.bits = (uint32_t *)((char *)ws + w.bits);
    p.B = B, p.T = o.maxT, p.U = o.maxU, p.V = V, p.blank = o.blank_label;
    p.Up = w.Up, p.NB = w.NB;
    p.divU = make_fastdiv((uint32_t)o.maxU);
}

rnntStatus_t get_rnnt_align_workspace_size(int maxT, int maxU, int minibatch, size_t *size_bytes) {
    if (!size_bytes || maxT <= 0 || maxU <= 0 || maxU > kMaxU || minibatch <= 0) return RNNT_STATUS_INVALID_VALUE;
    if ((long long)minibatch * maxT * maxU >= (1ll << 31)) return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = make_align_layout(maxT, maxU, minibatch).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_align_cells(const float *acts_slab, int slab_frames, int frame_offset, const int *flat_labels,
                                      const int *label_lengths, const int *input_lengths, int alphabet_size, int minibatch,
                                      void *workspace, rnntOptions options) {
    if (!acts_slab || !aligned4(acts_slab)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_align(flat_labels, label_lengths, input_lengths, workspace, alphabet_size, minibatch, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (slab_frames < 1 || frame_offset < 0 || (long long)frame_offset + slab_frames > options.maxT) return RNNT_STATUS_INVALID_VALUE;
    AlignParams p;
    fill_align(p, flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, workspace, options);
    p.acts = acts_slab, p.S = slab_frames, p.t0 = frame_offset;
    p.divS = make_fastdiv((uint32_t)slab_frames);
    return from_hip(launch_align_cells(p, (hipStream_t)options.stream));
}

// alphabet_size does not enter the sweep; the entry point takes none
rnntStatus_t compute_rnnt_align_path(int *token_frames, float *token_logp, float *scores, const int *label_lengths,
                                     const int *input_lengths, int minibatch, void *workspace, rnntOptions options) {
    if (!token_frames || !token_logp || !scores || !aligned4(token_frames) || !aligned4(token_logp) || !aligned4(scores))
        return RNNT_STATUS_INVALID_VALUE;
    // (the blank's range was checked against the vocabulary by the _cells calls that filled the workspace)
    const rnntStatus_t st =
        check_align(label_lengths, label_lengths, input_lengths, workspace, vocab_holding(options.blank_label), minibatch, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    AlignParams p;
    fill_align(p, nullptr, label_lengths, input_lengths, 0, minibatch, workspace, options);
    p.token_frames = token_frames, p.token_logp = token_logp, p.scores = scores;
    return from_hip(launch_align_path(p, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_align(const float *acts, const int *flat_labels, const int *label_lengths, const int *input_lengths,
                                int alphabet_size, int minibatch, int *token_frames, float *token_logp, float *scores,
                                void *workspace, rnntOptions options) {
    if (!acts || !aligned4(acts)) return RNNT_STATUS_INVALID_VALUE;
    if (!token_frames || !token_logp || !scores || !aligned4(token_frames) || !aligned4(token_logp) || !aligned4(scores))
        return RNNT_STATUS_INVALID_VALUE;
    rnntStatus_t st = check_align(flat_labels, label_lengths, input_lengths, workspace, alphabet_size, minibatch, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    st = compute_rnnt_align_cells(acts, options.maxT, 0, flat_labels, label_lengths, input_lengths, alphabet_size, minibatch,
                                  workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return compute_rnnt_align_path(token_frames, token_logp, scores, label_lengths, input_lengths, minibatch, workspace, options);
}

}  // extern "C"
