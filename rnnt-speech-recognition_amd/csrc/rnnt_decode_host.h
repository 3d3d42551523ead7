// rnnt_decode_host.h -- the host side of the decoders' extern "C" boundaries: the launchers of the greedy decoder, the beam search
// and their streams (greedy_kernels.hip, beam_kernels.hip), the argument checks every decoder entry point starts with, and the
// bodies of the unbiased beam steps.  Shared by rnnt_entrypoint.hip and by the entry points of the libraries that decode on the
// base kernels (bias, lm and the TDT decoders).  Everything here is checked before anything is enqueued.  No device code.
#pragma once
#include "rnnt_host.h"
#include "rnnt_common.h"

namespace rnnt {
// greedy_kernels.hip (batched greedy decoding)
hipError_t greedy_workspace_bytes(int T, int B, int J, int V, int joint_dtype, size_t *bytes);
hipError_t launch_greedy_begin(const float *enc_proj, const int *frame_lengths, const int *max_symbols, const float *W2,
                               const float *b2, int J, int V, int B, int T, int max_per_frame, int joint_dtype, void *workspace,
                               hipStream_t s);
hipError_t launch_greedy_step(const float *pred_proj, int *hyps, int max_hyp_len, int *hyp_lengths, float *scores, int *emitted,
                              int *all_done, float *stats, int *hyp_frames, float *hyp_logp, const int *frame_base, int J, int V,
                              int B, int T, int blank, int joint_dtype, void *workspace, hipStream_t s);
// beam_kernels.hip (batched modified beam search)
// (timed: the workspace layout with the {frame, log-probability} rows, and the kernels that keep them)
hipError_t beam_workspace_bytes(int T, int B, int K, int J, int V, int joint_dtype, bool timed, size_t *bytes);
hipError_t launch_beam_begin(const float *enc_proj, const int *frame_lengths, const float *W2, const float *b2, int J, int V, int B,
                             int T, int K, int joint_dtype, bool timed, void *workspace, hipStream_t s);
hipError_t launch_beam_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits, int *topk_symbols, float *lse,
                            int J, int V, int B, int T, int K, int N, int blank, int joint_dtype, bool timed, void *workspace,
                            hipStream_t s);
hipError_t launch_beam_results(int *hyps, int *hyp_lengths, float *scores, int *stable_lengths, int *hyp_frames, float *hyp_logp,
                               int *timed_stable_lengths, int J, int V, int B, int T, int K, int N, int joint_dtype, void *workspace,
                               hipStream_t s);
hipError_t beam_stream_workspace_bytes(int Tc, int S, int K, int N, int H, int J, int V, int joint_dtype, bool timed, size_t *bytes);
hipError_t launch_beam_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2, int H, int J, int V, int S,
                                    int Tc, int K, int N, int joint_dtype, bool timed, void *workspace, hipStream_t s);
hipError_t launch_beam_stream_feed(const float *enc, int Te, const int *chunk_frames, const int *reset, const int *final_, int H, int J,
                                   int V, int S, int Tc, int K, int N, int joint_dtype, bool timed, void *workspace, hipStream_t s);
// greedy_kernels.hip (streaming greedy decoding)
hipError_t greedy_stream_workspace_bytes(int Tc, int S, int H, int J, int V, int joint_dtype, size_t *bytes);
hipError_t launch_greedy_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2, int H, int J, int V, int S,
                                      int Tc, int joint_dtype, void *workspace, hipStream_t s);
hipError_t launch_greedy_stream_feed(const float *enc, int Te, const int *chunk_frames, const int *reset, const int *final_,
                                     const int *max_symbols, int max_per_frame, int *hyp_lengths, float *scores, int *all_done,
                                     int *frame_base, int H, int J, int V, int S, int Tc, int joint_dtype, void *workspace,
                                     hipStream_t s);
// tsd_stream_kernels.hip (the stream of the beam search with several symbols per frame; libwarprnnt_multibeamstream.so alone links it)
hipError_t tsd_stream_workspace_bytes(int Tc, int S, int K, int E, int N, int H, int J, int V, int joint_dtype, bool timed,
                                      size_t *bytes);
}  // namespace rnnt

static inline rnntStatus_t check_options(const rnntOptions &o) {
    if (o.loc != RNNT_GPU) return RNNT_STATUS_INVALID_VALUE;  // device-only library: no CPU fallback
    if (!o.batch_first) return RNNT_STATUS_INVALID_VALUE;
    if (o.maxT <= 0 || o.maxU <= 0 || o.blank_label < 0) return RNNT_STATUS_INVALID_VALUE;
    if (o.maxU > rnnt::kMaxU) return RNNT_STATUS_INVALID_VALUE;  // the wide sweep keeps two diagonals in LDS (include/rnnt.h)
    return RNNT_STATUS_SUCCESS;
}

// Batched greedy decoding (include/rnnt.h).
static inline rnntStatus_t check_greedy(int maxT, int joint_size, int alphabet_size, int minibatch, int joint_dtype,
                                        const rnntOptions &o) {
    if (joint_size <= 0 || alphabet_size <= 0 || minibatch <= 0 || maxT <= 0) return RNNT_STATUS_INVALID_VALUE;
    if (joint_dtype != 0 && joint_dtype != 1) return RNNT_STATUS_INVALID_VALUE;  // (RNNT_VISIT_ALL means nothing here: refused)
    const rnntStatus_t st = check_options(o);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (o.blank_label >= alphabet_size) return RNNT_STATUS_INVALID_VALUE;
    size_t n = 0;
    if (rnnt::greedy_workspace_bytes(maxT, minibatch, joint_size, alphabet_size, joint_dtype, &n) != hipSuccess)
        return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

// Batched beam search (include/rnnt.h).  The checks of the greedy decoder, plus 1 <= beam <= 16.
static inline rnntStatus_t check_beam(int maxT, int joint_size, int alphabet_size, int minibatch, int beam, int joint_dtype,
                                      const void *workspace, const rnntOptions &o, bool timed) {
    if (!workspace || ((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    if (beam < 1 || beam > 16) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_greedy(maxT, joint_size, alphabet_size, minibatch, joint_dtype, o);
    if (st != RNNT_STATUS_SUCCESS) return st;
    size_t n = 0;
    if (rnnt::beam_workspace_bytes(maxT, minibatch, beam, joint_size, alphabet_size, joint_dtype, timed, &n) != hipSuccess)
        return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

// Streaming greedy decoding (include/rnnt.h).
static inline rnntStatus_t check_greedy_stream(int max_chunk_frames, int slots, int enc_width, int joint_size, int alphabet_size,
                                               int joint_dtype, const void *workspace, const rnntOptions &o) {
    if (!workspace || ((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_greedy(max_chunk_frames, joint_size, alphabet_size, slots, joint_dtype, o);
    if (st != RNNT_STATUS_SUCCESS) return st;
    size_t n = 0;
    if (rnnt::greedy_stream_workspace_bytes(max_chunk_frames, slots, enc_width, joint_size, alphabet_size, joint_dtype, &n) !=
        hipSuccess)
        return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

// The beam stream (include/rnnt.h).  enc_width 1: step and results do not reach W1 / b1, which follow the beam workspace.
static inline rnntStatus_t check_beam_stream(int max_chunk_frames, int slots, int beam, int max_hyp_len, int enc_width,
                                             int joint_size, int alphabet_size, int joint_dtype, const void *workspace,
                                             const rnntOptions &o, bool timed) {
    if (!workspace || ((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    if (beam < 1 || beam > 16 || slots < 1 || (long long)slots * beam > 1024 || max_hyp_len < 1) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_greedy(max_chunk_frames, joint_size, alphabet_size, slots, joint_dtype, o);
    if (st != RNNT_STATUS_SUCCESS) return st;
    size_t n = 0;
    if (rnnt::beam_stream_workspace_bytes(max_chunk_frames, slots, beam, max_hyp_len, enc_width, joint_size, alphabet_size,
                                          joint_dtype, timed, &n) != hipSuccess)
        return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

// The stream of the beam search with several symbols per frame (include/rnnt_beam_multi_stream.h): the beam stream's checks on
// 2 beam rows per slot, symbols_per_frame in [1, 8], and the workspace's own layout.  enc_width 1: step and results do not reach
// W1 / b1, which stand last in the workspace.
static inline rnntStatus_t check_multibeam_stream(int max_chunk_frames, int slots, int beam, int symbols_per_frame, int max_hyp_len,
                                                  int enc_width, int joint_size, int alphabet_size, int joint_dtype,
                                                  const void *workspace, const rnntOptions &o, bool timed) {
    if (!workspace || ((uintptr_t)workspace & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    if (beam < 1 || beam > 16 || slots < 1 || (long long)slots * 2 * beam > 1024 || max_hyp_len < 1) return RNNT_STATUS_INVALID_VALUE;
    if (symbols_per_frame < 1 || symbols_per_frame > 8) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_greedy(max_chunk_frames, joint_size, alphabet_size, slots, joint_dtype, o);
    if (st != RNNT_STATUS_SUCCESS) return st;
    size_t n = 0;
    if (rnnt::tsd_stream_workspace_bytes(max_chunk_frames, slots, beam, symbols_per_frame, max_hyp_len, enc_width, joint_size,
                                         alphabet_size, joint_dtype, timed, &n) != hipSuccess)
        return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

static inline bool beam_step_pointers_aligned(const float *pred_proj, const int *parents, const int *emitted,
                                              const float *topk_logits, const int *topk_symbols, const float *lse) {
    return aligned4(pred_proj) && aligned4(parents) && aligned4(emitted) && aligned4(topk_logits) && aligned4(topk_symbols) &&
           aligned4(lse);
}

// The unbiased offline beam step: compute_rnnt_beam_step (timed false) and compute_rnnt_beam_timed_step, and what their biased
// and LM twins do on a NULL graph.
static inline rnntStatus_t beam_step_call(const float *pred_proj, int *parents, int *emitted, float *topk_logits, int *topk_symbols,
                                          float *lse, int joint_size, int alphabet_size, int minibatch, int beam, int joint_dtype,
                                          void *workspace, const rnntOptions &options, bool timed) {
    if (!pred_proj || !parents || !emitted) return RNNT_STATUS_INVALID_VALUE;
    // (the untimed offline step checks no alignment, as rnnt_entrypoint.hip's untimed begin and results)
    if (timed && !beam_step_pointers_aligned(pred_proj, parents, emitted, topk_logits, topk_symbols, lse))
        return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st =
        check_beam(options.maxT, joint_size, alphabet_size, minibatch, beam, joint_dtype, workspace, options, timed);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(rnnt::launch_beam_step(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, joint_size, alphabet_size,
                                           minibatch, options.maxT, beam, options.maxT, options.blank_label, joint_dtype, timed,
                                           workspace, (hipStream_t)options.stream));
}

// The unbiased step of the beam stream: compute_rnnt_beam_stream_step (timed false) and compute_rnnt_beam_stream_timed_step,
// and what their biased and LM twins do on a NULL graph.
static inline rnntStatus_t beam_stream_step_call(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                                 int *topk_symbols, float *lse, int joint_size, int alphabet_size, int slots,
                                                 int beam, int max_hyp_len, int joint_dtype, void *workspace,
                                                 const rnntOptions &options, bool timed) {
    if (!pred_proj || !parents || !emitted) return RNNT_STATUS_INVALID_VALUE;
    if (!beam_step_pointers_aligned(pred_proj, parents, emitted, topk_logits, topk_symbols, lse)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_beam_stream(options.maxT, slots, beam, max_hyp_len, 1, joint_size, alphabet_size, joint_dtype,
                                              workspace, options, timed);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return from_hip(rnnt::launch_beam_step(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, joint_size, alphabet_size,
                                           slots, options.maxT, beam, max_hyp_len, options.blank_label, joint_dtype, timed,
                                           workspace, (hipStream_t)options.stream));
}
