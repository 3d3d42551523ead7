// rnnt_tdt_stream_entrypoint.hip -- the extern "C" boundary of libwarprnnt_tdtstream.so (declared in include/rnnt_tdt_stream.h):
// greedy decoding of the token-and-duration (TDT) transducer over a stream of chunks per slot.  The other libraries and their
// headers stay as they are.  The argument checks of the greedy stream come from rnnt_decode_host.h and those of the batched TDT
// greedy decoder from tdt_host.h; this unit defines the four entry points and nothing else.  build.py links it with the base
// kernel objects, tdt_greedy_kernels.hip's object and tdt_stream_kernels.hip, and rnnt_tdt_stream.map exports the four entry
// points alone.
#include "tdt_host.h"
#include "../../include/rnnt_tdt_stream.h"

namespace rnnt {
// tdt_stream_kernels.hip
hipError_t tdt_stream_workspace_bytes(int Tc, int S, int H, int J, int Vt, int D, int joint_dtype, size_t *bytes);
hipError_t launch_tdt_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2, int H, int J, int Vt,
                                   const int *durations, int D, int S, int Tc, int joint_dtype, void *workspace, hipStream_t s);
hipError_t launch_tdt_stream_feed(const float *enc, int Te, const int *chunk_frames, const int *reset, const int *final_,
                                  const int *max_symbols, int max_per_frame, int *hyp_lengths, float *scores, int *all_done, int H,
                                  int J, int Vt, int D, int S, int Tc, int joint_dtype, void *workspace, hipStream_t s);
hipError_t launch_tdt_stream_step(const float *pred_proj, int *hyps, int *hyp_frames, float *hyp_logp, int max_hyp_len,
                                  int *hyp_lengths, float *scores, int *emitted, int *all_done, float *stats, int J, int Vt, int D,
                                  int S, int Tc, int blank, int joint_dtype, void *workspace, hipStream_t s);
}  // namespace rnnt

using namespace rnnt;

// the checks of the greedy stream at alphabet_size = R (the workspace pointer, the slots, the encoder width, the greedy decoder's
// own), then those of the TDT greedy decoder (the heads, the blank inside the token head) and the workspace's own layout
static rnntStatus_t check_tdt_stream(int max_chunk_frames, int slots, int enc_width, int joint_size, int alphabet_size,
                                     int num_durations, int joint_dtype, const void *workspace, const rnntOptions &o) {
    if (!tdt_heads_ok(alphabet_size, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    rnntStatus_t st = check_greedy_stream(max_chunk_frames, slots, enc_width, joint_size, alphabet_size + num_durations, joint_dtype,
                                          workspace, o);
    if (st != RNNT_STATUS_SUCCESS) return st;
    st = check_tdt_greedy(max_chunk_frames, joint_size, alphabet_size, num_durations, slots, joint_dtype, o);
    if (st != RNNT_STATUS_SUCCESS) return st;
    size_t n = 0;
    if (tdt_stream_workspace_bytes(max_chunk_frames, slots, enc_width, joint_size, alphabet_size, num_durations, joint_dtype, &n) !=
        hipSuccess)
        return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

extern "C" {

rnntStatus_t get_rnnt_tdt_greedy_stream_workspace_size(int max_chunk_frames, int slots, int enc_width, int joint_size,
                                                       int alphabet_size, int num_durations, int joint_dtype, size_t *size_bytes) {
    if (!size_bytes || !tdt_heads_ok(alphabet_size, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype != 0 && joint_dtype != 1) return RNNT_STATUS_INVALID_VALUE;
    if (joint_size <= 0 || slots <= 0 || max_chunk_frames <= 0) return RNNT_STATUS_INVALID_VALUE;
    return tdt_stream_workspace_bytes(max_chunk_frames, slots, enc_width, joint_size, alphabet_size, num_durations, joint_dtype,
                                      size_bytes) == hipSuccess
               ? RNNT_STATUS_SUCCESS
               : RNNT_STATUS_INVALID_VALUE;
}

rnntStatus_t compute_rnnt_tdt_greedy_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2, int enc_width,
                                                  int joint_size, int alphabet_size, const int *durations, int num_durations,
                                                  int slots, int joint_dtype, void *workspace, rnntOptions options) {
    if (!W1 || !b1 || !W2 || !b2 || !durations) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_tdt_stream(options.maxT, slots, enc_width, joint_size, alphabet_size, num_durations, joint_dtype,
                                             workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (!tdt_durations_ok(durations, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    return from_hip(launch_tdt_stream_begin(W1, b1, W2, b2, enc_width, joint_size, alphabet_size, durations, num_durations, slots,
                                            options.maxT, joint_dtype, workspace, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_tdt_greedy_stream_feed(const float *enc, int enc_frames, const int *chunk_frames, const int *reset,
                                                 const int *final_chunk, const int *max_symbols, int max_per_frame, int *hyp_lengths,
                                                 float *scores, int *all_done, int enc_width, int joint_size, int alphabet_size,
                                                 int num_durations, int slots, int joint_dtype, void *workspace, rnntOptions options) {
    if (!chunk_frames || !hyp_lengths || !scores || !all_done) return RNNT_STATUS_INVALID_VALUE;
    if (enc_frames < 0 || enc_frames > options.maxT || (enc_frames > 0 && !enc)) return RNNT_STATUS_INVALID_VALUE;
    if (max_per_frame < 1) return RNNT_STATUS_INVALID_VALUE;  // (with a duration 0 an uncapped decode need not end)
    const rnntStatus_t st = check_tdt_stream(options.maxT, slots, enc_width, joint_size, alphabet_size, num_durations, joint_dtype,
                                             workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_tdt_stream_feed(enc, enc_frames, chunk_frames, reset, final_chunk, max_symbols, max_per_frame, hyp_lengths,
                                           scores, all_done, enc_width, joint_size, alphabet_size, num_durations, slots, options.maxT,
                                           joint_dtype, workspace, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_tdt_greedy_stream_step(const float *pred_proj, int *hyps, int *hyp_frames, float *hyp_logp, int max_hyp_len,
                                                 int *hyp_lengths, float *scores, int *emitted, int *all_done, float *logit_stats,
                                                 int joint_size, int alphabet_size, int num_durations, int slots, int joint_dtype,
                                                 void *workspace, rnntOptions options) {
    if (!pred_proj || !hyps || !hyp_lengths || !scores || !emitted || !all_done) return RNNT_STATUS_INVALID_VALUE;
    if ((hyp_frames == nullptr) != (hyp_logp == nullptr)) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(hyps) || !aligned4(hyp_frames) || !aligned4(hyp_logp)) return RNNT_STATUS_INVALID_VALUE;
    if (max_hyp_len <= 0 || (long long)max_hyp_len * slots >= (1ll << 31)) return RNNT_STATUS_INVALID_VALUE;
    // (the step takes no enc_width: the stream's checks with a width of 1, which every layout takes)
    const rnntStatus_t st =
        check_tdt_stream(options.maxT, slots, 1, joint_size, alphabet_size, num_durations, joint_dtype, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(launch_tdt_stream_step(pred_proj, hyps, hyp_frames, hyp_logp, max_hyp_len, hyp_lengths, scores, emitted, all_done,
                                           logit_stats, joint_size, alphabet_size, num_durations, slots, options.maxT,
                                           options.blank_label, joint_dtype, workspace, (hipStream_t)options.stream));
}

}  // extern "C"
