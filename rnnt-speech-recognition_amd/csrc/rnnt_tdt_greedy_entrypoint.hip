// rnnt_tdt_greedy_entrypoint.hip -- the extern "C" boundary of libwarprnnt_tdtgreedy.so (declared in include/rnnt_tdt_greedy.h):
// batched greedy decoding of the token-and-duration (TDT) transducer.  libwarprnnt.so and include/rnnt.h, the base interface, stay
// as they are.  This translation unit includes rnnt_entrypoint.hip for the greedy decoder's argument checks (they are static
// there); build.py links it with the base kernel objects and tdt_greedy_kernels.hip, and rnnt_tdt_greedy.map keeps everything but
// the three entry points local, so the library defines no base entry point a second time.
#include "rnnt_entrypoint.hip"
#include "../../include/rnnt_tdt_greedy.h"

namespace rnnt {
// tdt_greedy_kernels.hip
hipError_t tdt_greedy_workspace_bytes(int T, int B, int J, int Vt, int D, int joint_dtype, size_t *bytes);
hipError_t launch_tdt_greedy_begin(const float *enc_proj, const int *frame_lengths, const int *max_symbols, const float *W2,
                                   const float *b2, int J, int Vt, const int *durations, int D, int B, int T, int max_per_frame,
                                   int joint_dtype, void *workspace, hipStream_t s);
hipError_t launch_tdt_greedy_step(const float *pred_proj, int *hyps, int *hyp_frames, float *hyp_logp, int max_hyp_len,
                                  int *hyp_lengths, float *scores, int *emitted, int *all_done, float *stats, int J, int Vt, int D,
                                  int B, int T, int blank, int joint_dtype, void *workspace, hipStream_t s);
}  // namespace rnnt

constexpr int kTdtGreedyMaxD = 8, kTdtGreedyMaxDuration = 8;  // include/rnnt_tdt.h's limits on the duration set

// 2 <= V, 1 <= D <= 8 (V + D cannot overflow: the greedy decoder takes no alphabet beyond 8192)
static bool tdt_heads_ok(int alphabet_size, int num_durations) {
    return alphabet_size >= 2 && alphabet_size <= (1 << 24) && num_durations >= 1 && num_durations <= kTdtGreedyMaxD;
}

// strictly increasing, durations[0] in {0, 1}, some d > 0, the largest <= 8
static bool tdt_durations_ok(const int *durations, int num_durations) {
    if (durations[0] != 0 && durations[0] != 1) return false;
    for (int i = 1; i < num_durations; ++i)
        if (durations[i] <= durations[i - 1]) return false;
    return durations[num_durations - 1] > 0 && durations[num_durations - 1] <= kTdtGreedyMaxDuration;
}

// the checks of the greedy decoder at alphabet_size = R, then the blank inside the token head and the workspace's own layout
static rnntStatus_t check_tdt_greedy(int maxT, int joint_size, int alphabet_size, int num_durations, int minibatch, int joint_dtype,
                                     const rnntOptions &o) {
    if (!tdt_heads_ok(alphabet_size, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_greedy(maxT, joint_size, alphabet_size + num_durations, minibatch, joint_dtype, o);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (o.blank_label >= alphabet_size) return RNNT_STATUS_INVALID_VALUE;
    size_t n = 0;
    if (tdt_greedy_workspace_bytes(maxT, minibatch, joint_size, alphabet_size, num_durations, joint_dtype, &n) != hipSuccess)
        return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

extern "C" {

rnntStatus_t get_rnnt_tdt_greedy_workspace_size(int maxT, int minibatch, int joint_size, int alphabet_size, int num_durations,
                                                int joint_dtype, size_t *size_bytes) {
    if (!size_bytes || !tdt_heads_ok(alphabet_size, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype != 0 && joint_dtype != 1) return RNNT_STATUS_INVALID_VALUE;
    if (joint_size <= 0 || minibatch <= 0 || maxT <= 0) return RNNT_STATUS_INVALID_VALUE;
    return tdt_greedy_workspace_bytes(maxT, minibatch, joint_size, alphabet_size, num_durations, joint_dtype, size_bytes) == hipSuccess
               ? RNNT_STATUS_SUCCESS
               : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t compute_rnnt_tdt_greedy_begin(const float *enc_proj, const int *frame_lengths, const int *max_symbols, const float *W2,
                                           const float *b2, int joint_size, int alphabet_size, const int *durations,
                                           int num_durations, int minibatch, int max_per_frame, int joint_dtype, void *workspace,
                                           rnntOptions options) {
    if (!enc_proj || !frame_lengths || !W2 || !b2 || !durations || !workspace) return RNNT_STATUS_INVALID_VALUE;
    if (max_per_frame < 1) return RNNT_STATUS_INVALID_VALUE;  // (with a duration 0 an uncapped decode need not end)
    const rnntStatus_t st =
        check_tdt_greedy(options.maxT, joint_size, alphabet_size, num_durations, minibatch, joint_dtype, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (!tdt_durations_ok(durations, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    return from_hip(launch_tdt_greedy_begin(enc_proj, frame_lengths, max_symbols, W2, b2, joint_size, alphabet_size, durations,
                                            num_durations, minibatch, options.maxT, max_per_frame, joint_dtype, workspace,
                                            (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_tdt_greedy_step(const float *pred_proj, int *hyps, int *hyp_frames, float *hyp_logp, int max_hyp_len,
                                          int *hyp_lengths, float *scores, int *emitted, int *all_done, float *logit_stats,
                                          int joint_size, int alphabet_size, int num_durations, int minibatch, int joint_dtype,
                                          void *workspace, rnntOptions options) {
    if (!pred_proj || !hyps || !hyp_lengths || !scores || !emitted || !all_done || !workspace) return RNNT_STATUS_INVALID_VALUE;
    if ((hyp_frames == nullptr) != (hyp_logp == nullptr)) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(hyps) || !aligned4(hyp_frames) || !aligned4(hyp_logp)) return RNNT_STATUS_INVALID_VALUE;
    if (max_hyp_len <= 0 || (long long)max_hyp_len * minibatch >= (1ll << 31)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st =
        check_tdt_greedy(options.maxT, joint_size, alphabet_size, num_durations, minibatch, joint_dtype, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    return from_hip(launch_tdt_greedy_step(pred_proj, hyps, hyp_frames, hyp_logp, max_hyp_len, hyp_lengths, scores, emitted, all_done,
                                           logit_stats, joint_size, alphabet_size, num_durations, minibatch, options.maxT,
                                           options.blank_label, joint_dtype, workspace, (hipStream_t)options.stream));
}

}  // extern "C"
