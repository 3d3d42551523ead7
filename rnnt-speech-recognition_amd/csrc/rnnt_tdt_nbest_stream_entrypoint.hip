// rnnt_tdt_nbest_stream_entrypoint.hip -- the extern "C" boundary of libwarprnnt_tdtbeamstream.so (declared in
// include/rnnt_tdt_beam_stream.h): chunked streaming beam search of the token-and-duration (TDT) transducer.  libwarprnnt.so and
// include/rnnt.h, the base interface, stay as they are.  The argument checks come from rnnt_decode_host.h (the beam
// stream's) and tdt_host.h (the TDT rules); this unit defines the five entry points and nothing else.  build.py links it with the
// base kernel objects and tdt_nbest_stream_kernels.hip, and rnnt_tdtbeamstream.map exports the five entry points alone.
#include "tdt_host.h"
#include "../../include/rnnt_tdt_beam_stream.h"

namespace rnnt {
// tdt_nbest_stream_kernels.hip
hipError_t tdt_beam_stream_workspace_bytes(int Tc, int S, int K, int N, int H, int J, int Vt, int D, int joint_dtype, bool timed,
                                           size_t *bytes);
hipError_t launch_tdt_beam_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2, int H, int J, int Vt,
                                        const int *durations, int D, int S, int Tc, int K, int N, int joint_dtype, bool timed,
                                        void *workspace, hipStream_t s);
hipError_t launch_tdt_beam_stream_feed(const float *enc, int Te, const int *chunk_frames, const int *reset, const int *final_, int H,
                                       int J, int Vt, int D, int S, int Tc, int K, int N, int joint_dtype, bool timed, void *workspace,
                                       hipStream_t s);
hipError_t launch_tdt_beam_stream_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits, int *topk_symbols,
                                       float *dur_logits, float *lse, int J, int Vt, int D, int S, int Tc, int K, int N, int blank,
                                       int joint_dtype, bool timed, void *workspace, hipStream_t s);
hipError_t launch_tdt_beam_stream_results(int *hyps, int *hyp_lengths, float *scores, int *cursors, int *stable_lengths,
                                          int *hyp_frames, int *hyp_durations, int *timed_stable_lengths, int J, int Vt, int D, int S,
                                          int Tc, int K, int N, int joint_dtype, bool timed, void *workspace, hipStream_t s);
}  // namespace rnnt

using namespace rnnt;

// the checks of the beam stream at alphabet_size = R, then the blank inside the token head and the workspace's own layout.
// enc_width 1: step and results do not reach W1 / b1.
static rnntStatus_t check_tdt_beam_stream(int max_chunk_frames, int slots, int beam, int max_hyp_len, int enc_width, int joint_size,
                                          int alphabet_size, int num_durations, int joint_dtype, bool timed, const void *workspace,
                                          const rnntOptions &o) {
    if (!tdt_heads_ok(alphabet_size, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_beam_stream(max_chunk_frames, slots, beam, max_hyp_len, enc_width, joint_size,
                                              alphabet_size + num_durations, joint_dtype, workspace, o, timed);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (o.blank_label >= alphabet_size) return RNNT_STATUS_INVALID_VALUE;
    size_t n = 0;
    if (tdt_beam_stream_workspace_bytes(max_chunk_frames, slots, beam, max_hyp_len, enc_width, joint_size, alphabet_size, num_durations,
                                        joint_dtype, timed, &n) != hipSuccess)
        return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

extern "C" {

rnntStatus_t get_rnnt_tdt_beam_stream_workspace_size(int max_chunk_frames, int slots, int beam, int max_hyp_len, int enc_width,
                                                     int joint_size, int alphabet_size, int num_durations, int joint_dtype, int timed,
                                                     size_t *size_bytes) {
    if (!size_bytes || !tdt_heads_ok(alphabet_size, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype != 0 && joint_dtype != 1) return RNNT_STATUS_INVALID_VALUE;
    if (joint_size <= 0 || slots <= 0 || max_chunk_frames <= 0 || beam < 1 || beam > 16 || max_hyp_len < 1)
        return RNNT_STATUS_INVALID_VALUE;
    return tdt_beam_stream_workspace_bytes(max_chunk_frames, slots, beam, max_hyp_len, enc_width, joint_size, alphabet_size,
                                           num_durations, joint_dtype, timed != 0, size_bytes) == hipSuccess
               ? RNNT_STATUS_SUCCESS
               : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t compute_rnnt_tdt_beam_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2, int enc_width,
                                                int joint_size, int alphabet_size, const int *durations, int num_durations, int slots,
                                                int beam, int max_hyp_len, int joint_dtype, int timed, void *workspace,
                                                rnntOptions options) {
    if (!W1 || !b1 || !W2 || !b2 || !durations) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(W1) || !aligned4(b1) || !aligned4(W2) || !aligned4(b2)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_tdt_beam_stream(options.maxT, slots, beam, max_hyp_len, enc_width, joint_size, alphabet_size,
                                                  num_durations, joint_dtype, timed != 0, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (!tdt_durations_ok(durations, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    return from_hip(launch_tdt_beam_stream_begin(W1, b1, W2, b2, enc_width, joint_size, alphabet_size, durations, num_durations, slots,
                                                 options.maxT, beam, max_hyp_len, joint_dtype, timed != 0, workspace,
                                                 (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_tdt_beam_stream_feed(const float *enc, int enc_frames, const int *chunk_frames, const int *reset,
                                               const int *final_chunk, int enc_width, int joint_size, int alphabet_size,
                                               int num_durations, int slots, int beam, int max_hyp_len, int joint_dtype, int timed,
                                               void *workspace, rnntOptions options) {
    if (!chunk_frames || !aligned4(enc) || !aligned4(chunk_frames) || !aligned4(reset) || !aligned4(final_chunk))
        return RNNT_STATUS_INVALID_VALUE;
    if (enc_frames < 0 || enc_frames > options.maxT || (enc_frames > 0 && !enc)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_tdt_beam_stream(options.maxT, slots, beam, max_hyp_len, enc_width, joint_size, alphabet_size,
                                                  num_durations, joint_dtype, timed != 0, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_tdt_beam_stream_feed(enc, enc_frames, chunk_frames, reset, final_chunk, enc_width, joint_size, alphabet_size,
                                                num_durations, slots, options.maxT, beam, max_hyp_len, joint_dtype, timed != 0,
                                                workspace, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_tdt_beam_stream_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                               int *topk_symbols, float *dur_logits, float *lse, int joint_size, int alphabet_size,
                                               int num_durations, int slots, int beam, int max_hyp_len, int joint_dtype, int timed,
                                               void *workspace, rnntOptions options) {
    if (!pred_proj || !parents || !emitted) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(pred_proj) || !aligned4(parents) || !aligned4(emitted) || !aligned4(topk_logits) || !aligned4(topk_symbols) ||
        !aligned4(dur_logits) || !aligned4(lse))
        return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_tdt_beam_stream(options.maxT, slots, beam, max_hyp_len, 1, joint_size, alphabet_size,
                                                  num_durations, joint_dtype, timed != 0, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_tdt_beam_stream_step(pred_proj, parents, emitted, topk_logits, topk_symbols, dur_logits, lse, joint_size,
                                                alphabet_size, num_durations, slots, options.maxT, beam, max_hyp_len,
                                                options.blank_label, joint_dtype, timed != 0, workspace,
                                                (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_tdt_beam_stream_results(int *hyps, int *hyp_lengths, float *scores, int *cursors, int *stable_lengths,
                                                  int *hyp_frames, int *hyp_durations, int *timed_stable_lengths, int joint_size,
                                                  int alphabet_size, int num_durations, int slots, int beam, int max_hyp_len,
                                                  int joint_dtype, int timed, void *workspace, rnntOptions options) {
    if (!hyps || !hyp_lengths || !scores) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(hyps) || !aligned4(hyp_lengths) || !aligned4(scores) || !aligned4(cursors) || !aligned4(stable_lengths) ||
        !aligned4(hyp_frames) || !aligned4(hyp_durations) || !aligned4(timed_stable_lengths))
        return RNNT_STATUS_INVALID_VALUE;
    if ((hyp_frames == nullptr) != (hyp_durations == nullptr)) return RNNT_STATUS_INVALID_VALUE;
    if ((hyp_frames || timed_stable_lengths) && timed == 0) return RNNT_STATUS_INVALID_VALUE;  // (a timed workspace alone holds the rows)
    const rnntStatus_t st = check_tdt_beam_stream(options.maxT, slots, beam, max_hyp_len, 1, joint_size, alphabet_size,
                                                  num_durations, joint_dtype, timed != 0, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_tdt_beam_stream_results(hyps, hyp_lengths, scores, cursors, stable_lengths, hyp_frames, hyp_durations,
                                                   timed_stable_lengths, joint_size, alphabet_size, num_durations, slots, options.maxT,
                                                   beam, max_hyp_len, joint_dtype, timed != 0, workspace,
                                                   (hipStream_t)options.stream));
}

}  // extern "C"
