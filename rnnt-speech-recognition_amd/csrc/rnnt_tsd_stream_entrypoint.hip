// rnnt_tsd_stream_entrypoint.hip -- the extern "C" boundary of libwarprnnt_multibeamstream.so (declared in
// include/rnnt_beam_multi_stream.h): chunked streaming beam search with several symbols per frame.  libwarprnnt.so and
// include/rnnt.h, the base interface, stay as they are.  The argument checks are in rnnt_decode_host.h beside the other
// decoders'; this unit defines the five entry points and nothing else.  build.py links it with the base kernel objects and
// tsd_stream_kernels.hip, and rnnt_tsdstream.map exports the five entry points alone.
#include "rnnt_decode_host.h"
#include "../../include/rnnt_beam_multi_stream.h"

namespace rnnt {
// tsd_stream_kernels.hip
hipError_t launch_tsd_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2, int H, int J, int V, int S,
                                   int Tc, int K, int E, int N, int joint_dtype, bool timed, void *workspace, hipStream_t s);
hipError_t launch_tsd_stream_feed(const float *enc, int Te, const int *chunk_frames, const int *reset, const int *final_, int H, int J,
                                  int V, int S, int Tc, int K, int E, int N, int joint_dtype, bool timed, void *workspace,
                                  hipStream_t s);
hipError_t launch_tsd_stream_step(const float *pred_proj, int *parents, int *emitted, int J, int V, int S, int Tc, int K, int E, int N,
                                  int blank, int joint_dtype, bool timed, void *workspace, hipStream_t s);
hipError_t launch_tsd_stream_results(int *hyps, int *hyp_lengths, float *scores, int *stable_lengths, int *hyp_frames,
                                     int *timed_stable_lengths, int J, int V, int S, int Tc, int K, int E, int N, int joint_dtype,
                                     bool timed, void *workspace, hipStream_t s);
}  // namespace rnnt

using namespace rnnt;

extern "C" {

rnntStatus_t get_rnnt_multibeam_stream_workspace_size(int max_chunk_frames, int slots, int beam, int symbols_per_frame,
                                                      int max_hyp_len, int enc_width, int joint_size, int alphabet_size,
                                                      int joint_dtype, int timed, size_t *size_bytes) {
    if (!size_bytes) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype != 0 && joint_dtype != 1) return RNNT_STATUS_INVALID_VALUE;
    if (joint_size <= 0 || alphabet_size <= 0 || slots <= 0 || max_chunk_frames <= 0 || beam < 1 || beam > 16 || max_hyp_len < 1)
        return RNNT_STATUS_INVALID_VALUE;
    if (symbols_per_frame < 1 || symbols_per_frame > 8 || (long long)slots * 2 * beam > 1024) return RNNT_STATUS_INVALID_VALUE;
    return tsd_stream_workspace_bytes(max_chunk_frames, slots, beam, symbols_per_frame, max_hyp_len, enc_width, joint_size,
                                      alphabet_size, joint_dtype, timed != 0, size_bytes) == hipSuccess
               ? RNNT_STATUS_SUCCESS
               : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t compute_rnnt_multibeam_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2, int enc_width,
                                                 int joint_size, int alphabet_size, int slots, int beam, int symbols_per_frame,
                                                 int max_hyp_len, int joint_dtype, int timed, void *workspace, rnntOptions options) {
    if (!W1 || !b1 || !W2 || !b2) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(W1) || !aligned4(b1) || !aligned4(W2) || !aligned4(b2)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_multibeam_stream(options.maxT, slots, beam, symbols_per_frame, max_hyp_len, enc_width, joint_size,
                                                   alphabet_size, joint_dtype, workspace, options, timed != 0);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_tsd_stream_begin(W1, b1, W2, b2, enc_width, joint_size, alphabet_size, slots, options.maxT, beam,
                                            symbols_per_frame, max_hyp_len, joint_dtype, timed != 0, workspace,
                                            (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_multibeam_stream_feed(const float *enc, int enc_frames, const int *chunk_frames, const int *reset,
                                                const int *final_chunk, int enc_width, int joint_size, int alphabet_size, int slots,
                                                int beam, int symbols_per_frame, int max_hyp_len, int joint_dtype, int timed,
                                                void *workspace, rnntOptions options) {
    if (!chunk_frames || !aligned4(enc) || !aligned4(chunk_frames) || !aligned4(reset) || !aligned4(final_chunk))
        return RNNT_STATUS_INVALID_VALUE;
    if (enc_frames < 0 || enc_frames > options.maxT || (enc_frames > 0 && !enc)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_multibeam_stream(options.maxT, slots, beam, symbols_per_frame, max_hyp_len, enc_width, joint_size,
                                                   alphabet_size, joint_dtype, workspace, options, timed != 0);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_tsd_stream_feed(enc, enc_frames, chunk_frames, reset, final_chunk, enc_width, joint_size, alphabet_size,
                                           slots, options.maxT, beam, symbols_per_frame, max_hyp_len, joint_dtype, timed != 0,
                                           workspace, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_multibeam_stream_step(const float *pred_proj, int *parents, int *emitted, int joint_size, int alphabet_size,
                                                int slots, int beam, int symbols_per_frame, int max_hyp_len, int joint_dtype,
                                                int timed, void *workspace, rnntOptions options) {
    if (!pred_proj || !parents || !emitted) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(pred_proj) || !aligned4(parents) || !aligned4(emitted)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_multibeam_stream(options.maxT, slots, beam, symbols_per_frame, max_hyp_len, 1, joint_size,
                                                   alphabet_size, joint_dtype, workspace, options, timed != 0);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_tsd_stream_step(pred_proj, parents, emitted, joint_size, alphabet_size, slots, options.maxT, beam,
                                           symbols_per_frame, max_hyp_len, options.blank_label, joint_dtype, timed != 0, workspace,
                                           (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_multibeam_stream_results(int *hyps, int *hyp_lengths, float *scores, int *stable_lengths, int *hyp_frames,
                                                   int *timed_stable_lengths, int joint_size, int alphabet_size, int slots, int beam,
                                                   int symbols_per_frame, int max_hyp_len, int joint_dtype, int timed, void *workspace,
                                                   rnntOptions options) {
    if (!hyps || !hyp_lengths || !scores) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(hyps) || !aligned4(hyp_lengths) || !aligned4(scores) || !aligned4(stable_lengths) || !aligned4(hyp_frames) ||
        !aligned4(timed_stable_lengths))
        return RNNT_STATUS_INVALID_VALUE;
    if ((hyp_frames || timed_stable_lengths) && timed == 0) return RNNT_STATUS_INVALID_VALUE;  // (a timed workspace alone holds the rows)
    const rnntStatus_t st = check_multibeam_stream(options.maxT, slots, beam, symbols_per_frame, max_hyp_len, 1, joint_size,
                                                   alphabet_size, joint_dtype, workspace, options, timed != 0);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_tsd_stream_results(hyps, hyp_lengths, scores, stable_lengths, hyp_frames, timed_stable_lengths, joint_size,
                                              alphabet_size, slots, options.maxT, beam, symbols_per_frame, max_hyp_len, joint_dtype,
                                              timed != 0, workspace, (hipStream_t)options.stream));
}

}  // extern "C"
