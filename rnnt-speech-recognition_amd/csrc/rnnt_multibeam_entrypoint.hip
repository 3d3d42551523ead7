// rnnt_multibeam_entrypoint.hip -- the extern "C" boundary of libwarprnnt_multibeam.so (declared in include/rnnt_beam_multi.h):
// batched beam search with several symbols per frame.  libwarprnnt.so and include/rnnt.h, the base interface, stay as they are.
// The argument checks are the beam search's (rnnt_decode_host.h) and the three of this header; this unit defines the four entry
// points and nothing else.  build.py links it with the base kernel objects and multibeam_kernels.hip, and rnnt_multibeam.map
// exports the four entry points alone.
#include "rnnt_decode_host.h"
#include "../../include/rnnt_beam_multi.h"

namespace rnnt {
// multibeam_kernels.hip
hipError_t multibeam_workspace_bytes(int T, int B, int K, int E, int N, int J, int V, int joint_dtype, size_t *bytes);
hipError_t launch_multibeam_begin(const float *enc_proj, const int *frame_lengths, const float *W2, const float *b2, int J, int V,
                                  int B, int T, int K, int E, int N, int joint_dtype, void *workspace, hipStream_t s);
hipError_t launch_multibeam_step(const float *pred_proj, int *parents, int *emitted, int J, int V, int B, int T, int K, int E, int N,
                                 int blank, int joint_dtype, void *workspace, hipStream_t s);
hipError_t launch_multibeam_results(int *hyps, int *hyp_lengths, float *scores, int J, int V, int B, int T, int K, int E, int N,
                                    int joint_dtype, void *workspace, hipStream_t s);
}  // namespace rnnt

using namespace rnnt;

// symbols_per_frame in [1, 8], max_hyp_len >= 1, minibatch 2 beam <= 1024 rows (1 <= beam <= 16, minibatch >= 1)
static bool multibeam_sizes_ok(int minibatch, int beam, int symbols_per_frame, int max_hyp_len) {
    if (symbols_per_frame < 1 || symbols_per_frame > 8 || max_hyp_len < 1) return false;
    return minibatch >= 1 && beam >= 1 && beam <= 16 && (long long)minibatch * 2 * beam <= 1024;
}

// the checks of the beam search, then this search's sizes and the workspace's own layout
static rnntStatus_t check_multibeam(int maxT, int joint_size, int alphabet_size, int minibatch, int beam, int symbols_per_frame,
                                    int max_hyp_len, int joint_dtype, const void *workspace, const rnntOptions &o) {
    if (!multibeam_sizes_ok(minibatch, beam, symbols_per_frame, max_hyp_len)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_beam(maxT, joint_size, alphabet_size, minibatch, beam, joint_dtype, workspace, o, false);
    if (st != RNNT_STATUS_SUCCESS) return st;
    size_t n = 0;
    if (multibeam_workspace_bytes(maxT, minibatch, beam, symbols_per_frame, max_hyp_len, joint_size, alphabet_size, joint_dtype, &n) !=
        hipSuccess)
        return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

extern "C" {

rnntStatus_t get_rnnt_multibeam_workspace_size(int maxT, int minibatch, int beam, int symbols_per_frame, int max_hyp_len,
                                               int joint_size, int alphabet_size, int joint_dtype, size_t *size_bytes) {
    if (!size_bytes || !multibeam_sizes_ok(minibatch, beam, symbols_per_frame, max_hyp_len)) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype != 0 && joint_dtype != 1) return RNNT_STATUS_INVALID_VALUE;
    if (joint_size <= 0 || alphabet_size <= 0 || maxT <= 0) return RNNT_STATUS_INVALID_VALUE;
    return multibeam_workspace_bytes(maxT, minibatch, beam, symbols_per_frame, max_hyp_len, joint_size, alphabet_size, joint_dtype,
                                     size_bytes) == hipSuccess
               ? RNNT_STATUS_SUCCESS
               : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t compute_rnnt_multibeam_begin(const float *enc_proj, const int *frame_lengths, const float *W2, const float *b2,
                                          int joint_size, int alphabet_size, int minibatch, int beam, int symbols_per_frame,
                                          int max_hyp_len, int joint_dtype, void *workspace, rnntOptions options) {
    if (!enc_proj || !frame_lengths || !W2 || !b2) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_multibeam(options.maxT, joint_size, alphabet_size, minibatch, beam, symbols_per_frame, max_hyp_len,
                                            joint_dtype, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_multibeam_begin(enc_proj, frame_lengths, W2, b2, joint_size, alphabet_size, minibatch, options.maxT, beam,
                                           symbols_per_frame, max_hyp_len, joint_dtype, workspace, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_multibeam_step(const float *pred_proj, int *parents, int *emitted, int joint_size, int alphabet_size,
                                         int minibatch, int beam, int symbols_per_frame, int max_hyp_len, int joint_dtype,
                                         void *workspace, rnntOptions options) {
    if (!pred_proj || !parents || !emitted) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_multibeam(options.maxT, joint_size, alphabet_size, minibatch, beam, symbols_per_frame, max_hyp_len,
                                            joint_dtype, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_multibeam_step(pred_proj, parents, emitted, joint_size, alphabet_size, minibatch, options.maxT, beam,
                                          symbols_per_frame, max_hyp_len, options.blank_label, joint_dtype, workspace,
                                          (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_multibeam_results(int *hyps, int *hyp_lengths, float *scores, int joint_size, int alphabet_size,
                                            int minibatch, int beam, int symbols_per_frame, int max_hyp_len, int joint_dtype,
                                            void *workspace, rnntOptions options) {
    if (!hyps || !hyp_lengths || !scores) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_multibeam(options.maxT, joint_size, alphabet_size, minibatch, beam, symbols_per_frame, max_hyp_len,
                                            joint_dtype, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_multibeam_results(hyps, hyp_lengths, scores, joint_size, alphabet_size, minibatch, options.maxT, beam,
                                             symbols_per_frame, max_hyp_len, joint_dtype, workspace, (hipStream_t)options.stream));
}

}  // extern "C"
