// rnnt_tdt_beam_entrypoint.hip -- the extern "C" boundary of libwarprnnt_tdtbeam.so (declared in include/rnnt_tdt_beam.h): batched beam
// search of the token-and-duration (TDT) transducer.  libwarprnnt.so and include/rnnt.h, the base interface, stay as they are.  The
// argument checks come from rnnt_decode_host.h (the beam search's) and tdt_host.h (the TDT rules); this unit defines the four entry
// points and nothing else.  build.py links it with the base kernel objects and tdt_beam_kernels.hip, and rnnt_tdtbeam.map exports
// the four entry points alone.
#include "tdt_host.h"
#include "../../include/rnnt_tdt_beam.h"

namespace rnnt {
// tdt_beam_kernels.hip
hipError_t tdt_beam_workspace_bytes(int T, int B, int K, int J, int Vt, int D, int joint_dtype, bool timed, size_t *bytes);
hipError_t launch_tdt_beam_begin(const float *enc_proj, const int *frame_lengths, const float *W2, const float *b2, int J, int Vt,
                                 const int *durations, int D, int B, int T, int K, int joint_dtype, bool timed, void *workspace,
                                 hipStream_t s);
hipError_t launch_tdt_beam_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits, int *topk_symbols,
                                float *dur_logits, float *lse, int J, int Vt, int D, int B, int T, int K, int blank, int joint_dtype,
                                bool timed, void *workspace, hipStream_t s);
hipError_t launch_tdt_beam_results(int *hyps, int *hyp_lengths, float *scores, int *cursors, int *hyp_frames, int *hyp_durations,
                                   int J, int Vt, int D, int B, int T, int K, int joint_dtype, bool timed, void *workspace,
                                   hipStream_t s);
}  // namespace rnnt

using namespace rnnt;

// the checks of the beam search at alphabet_size = R, then the blank inside the token head and the workspace's own layout
static rnntStatus_t check_tdt_beam(int maxT, int joint_size, int alphabet_size, int num_durations, int minibatch, int beam,
                                   int joint_dtype, bool timed, const void *workspace, const rnntOptions &o) {
    if (!tdt_heads_ok(alphabet_size, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_beam(maxT, joint_size, alphabet_size + num_durations, minibatch, beam, joint_dtype, workspace, o, timed);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (o.blank_label >= alphabet_size) return RNNT_STATUS_INVALID_VALUE;
    size_t n = 0;
    if (tdt_beam_workspace_bytes(maxT, minibatch, beam, joint_size, alphabet_size, num_durations, joint_dtype, timed, &n) != hipSuccess)
        return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

extern "C" {

rnntStatus_t get_rnnt_tdt_beam_workspace_size(int maxT, int minibatch, int beam, int joint_size, int alphabet_size, int num_durations,
                                              int joint_dtype, int timed, size_t *size_bytes) {
    if (!size_bytes || !tdt_heads_ok(alphabet_size, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype != 0 && joint_dtype != 1) return RNNT_STATUS_INVALID_VALUE;
    if (joint_size <= 0 || minibatch <= 0 || maxT <= 0 || beam < 1 || beam > 16) return RNNT_STATUS_INVALID_VALUE;
    return tdt_beam_workspace_bytes(maxT, minibatch, beam, joint_size, alphabet_size, num_durations, joint_dtype, timed != 0,
                                    size_bytes) == hipSuccess
               ? RNNT_STATUS_SUCCESS
               : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t compute_rnnt_tdt_beam_begin(const float *enc_proj, const int *frame_lengths, const float *W2, const float *b2,
                                         int joint_size, int alphabet_size, const int *durations, int num_durations, int minibatch,
                                         int beam, int joint_dtype, int timed, void *workspace, rnntOptions options) {
    if (!enc_proj || !frame_lengths || !W2 || !b2 || !durations) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_tdt_beam(options.maxT, joint_size, alphabet_size, num_durations, minibatch, beam, joint_dtype,
                                           timed != 0, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (!tdt_durations_ok(durations, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    return from_hip(launch_tdt_beam_begin(enc_proj, frame_lengths, W2, b2, joint_size, alphabet_size, durations, num_durations,
                                          minibatch, options.maxT, beam, joint_dtype, timed != 0, workspace,
                                          (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_tdt_beam_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits, int *topk_symbols,
                                        float *dur_logits, float *lse, int joint_size, int alphabet_size, int num_durations,
                                        int minibatch, int beam, int joint_dtype, int timed, void *workspace, rnntOptions options) {
    if (!pred_proj || !parents || !emitted) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_tdt_beam(options.maxT, joint_size, alphabet_size, num_durations, minibatch, beam, joint_dtype,
                                           timed != 0, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_tdt_beam_step(pred_proj, parents, emitted, topk_logits, topk_symbols, dur_logits, lse, joint_size,
                                         alphabet_size, num_durations, minibatch, options.maxT, beam, options.blank_label, joint_dtype,
                                         timed != 0, workspace, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_tdt_beam_results(int *hyps, int *hyp_lengths, float *scores, int *cursors, int *hyp_frames,
                                           int *hyp_durations, int joint_size, int alphabet_size, int num_durations, int minibatch,
                                           int beam, int joint_dtype, int timed, void *workspace, rnntOptions options) {
    if (!hyps || !hyp_lengths || !scores) return RNNT_STATUS_INVALID_VALUE;
    if ((hyp_frames == nullptr) != (hyp_durations == nullptr)) return RNNT_STATUS_INVALID_VALUE;
    if (hyp_frames && timed == 0) return RNNT_STATUS_INVALID_VALUE;  // (the rows exist in a timed workspace alone)
    const rnntStatus_t st = check_tdt_beam(options.maxT, joint_size, alphabet_size, num_durations, minibatch, beam, joint_dtype,
                                           timed != 0, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_tdt_beam_results(hyps, hyp_lengths, scores, cursors, hyp_frames, hyp_durations, joint_size, alphabet_size,
                                            num_durations, minibatch, options.maxT, beam, joint_dtype, timed != 0, workspace,
                                            (hipStream_t)options.stream));
}

}  // extern "C"
