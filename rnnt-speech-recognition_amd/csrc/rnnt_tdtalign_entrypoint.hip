// rnnt_tdtalign_entrypoint.hip -- the extern "C" boundary of libwarprnnt_tdtalign.so (declared in include/rnnt_tdt_align.h): forced
// alignment on the token-and-duration (TDT) lattice.  The other libraries and their headers stay as they are.  build.py links this
// translation unit with rnnt_tdtalign_kernels.hip alone, and rnnt_tdtalign.map keeps everything but the four entry points local.
// Argument validation follows compute_rnnt_loss_tdt's and compute_rnnt_modified_align's: everything is checked before anything is
// enqueued, nothing is allocated, everything is enqueued on the caller's stream.
#include "../../include/rnnt_tdt_align.h"
#include "rnnt_tdtalign.h"
#include "tdt_host.h"

#include <math.h>

using namespace rnnt;

// the shape limits of the op (include/rnnt_tdt_align.h): maxU <= 1024, minibatch * maxT * maxU < 2^31, 1 <= num_durations <= 8
static bool shape_ok(int maxT, int maxU, int minibatch, int num_durations) {
    if (maxT <= 0 || maxU <= 0 || maxU > kTdtAlignMaxU || minibatch <= 0) return false;
    if (num_durations < 1 || num_durations > kTdtAlignMaxD) return false;
    return (long long)minibatch * maxT * maxU < (1ll << 31);
}

// what _cells and _path share: V = the token vocabulary (_path: anything that holds the blank)
static rnntStatus_t check_common(const void *ll, const void *il, const int *durations, int D, const void *ws, int V, int B,
                                 const rnntOptions &o) {
    if (!ll || !il || !durations || !ws) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(ll) || !aligned4(il)) return RNNT_STATUS_INVALID_VALUE;
    if (o.loc != RNNT_GPU || !o.batch_first) return RNNT_STATUS_INVALID_VALUE;  // device-only library: no CPU fallback
    if (V < 2 || o.blank_label < 0 || o.blank_label >= V) return RNNT_STATUS_INVALID_VALUE;
    if (!shape_ok(o.maxT, o.maxU, B, D)) return RNNT_STATUS_INVALID_VALUE;
    if (!tdt_durations_ok(durations, D)) return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)ws & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

static bool outputs_ok(const int *frames, const int *durs, const float *logp, const float *scores) {
    return frames && durs && logp && scores && aligned4(frames) && aligned4(durs) && aligned4(logp) && aligned4(scores);
}

static TdtAlignParams make_params(const int *ll, const int *il, const int *durations, int D, int B, void *ws, const rnntOptions &o) {
    const TdtAlignLayout w = make_tdtalign_layout(o.maxT, o.maxU, B, D);
    TdtAlignParams p{};
    p.label_lengths = ll, p.input_lengths = il;
    p.sigma_slot = (float *)((char *)ws + w.sigma);
    p.w = (float *)((char *)ws + w.w);
    p.dec = (uint8_t *)((char *)ws + w.dec);
    p.B = B, p.T = o.maxT, p.U = o.maxU, p.D = D, p.blank = o.blank_label;
    p.Up = w.Up, p.N = w.N;
    for (int i = 0; i < kTdtAlignMaxD; ++i) {
        p.dur[i] = i < D ? durations[i] : 0;
        p.dur_packed |= (uint32_t)p.dur[i] << (4 * i);
    }
    p.divU = make_fastdiv((uint32_t)o.maxU);
    return p;
}

extern "C" {

rnntStatus_t get_rnnt_tdt_align_workspace_size(int maxT, int maxU, int minibatch, int num_durations, size_t *size_bytes) {
    if (!size_bytes || !shape_ok(maxT, maxU, minibatch, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = make_tdtalign_layout(maxT, maxU, minibatch, num_durations).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_tdt_align_cells(const float *acts_slab, int slab_frames, int frame_offset, const int *flat_labels,
                                          const int *label_lengths, const int *input_lengths, int alphabet_size, const int *durations,
                                          int num_durations, float sigma, int minibatch, void *workspace, rnntOptions options) {
    if (!(sigma >= 0.f) || !isfinite(sigma)) return RNNT_STATUS_INVALID_VALUE;  // (NaN fails the first)
    if (!acts_slab || !aligned4(acts_slab) || !flat_labels || !aligned4(flat_labels)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_common(label_lengths, input_lengths, durations, num_durations, workspace, alphabet_size, minibatch, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (slab_frames < 1 || frame_offset < 0 || (long long)frame_offset + slab_frames > options.maxT) return RNNT_STATUS_INVALID_VALUE;
    TdtAlignParams p = make_params(label_lengths, input_lengths, durations, num_durations, minibatch, workspace, options);
    p.acts = acts_slab, p.labels = flat_labels, p.V = alphabet_size, p.sigma = sigma;
    p.S = slab_frames, p.t0 = frame_offset;
    p.divS = make_fastdiv((uint32_t)slab_frames);
    return from_hip(launch_tdtalign_cells(p, (hipStream_t)options.stream));
}

// alphabet_size and sigma do not enter the sweep; the entry point takes neither (sigma comes back from the workspace)
rnntStatus_t compute_rnnt_tdt_align_path(int *token_frames, int *token_durations, float *token_logp, float *scores,
                                         const int *label_lengths, const int *input_lengths, const int *durations, int num_durations,
                                         int minibatch, void *workspace, rnntOptions options) {
    if (!outputs_ok(token_frames, token_durations, token_logp, scores)) return RNNT_STATUS_INVALID_VALUE;
    // (the blank's range was checked against the vocabulary by the _cells calls that filled the workspace)
    const rnntStatus_t st = check_common(label_lengths, input_lengths, durations, num_durations, workspace,
                                         vocab_holding(options.blank_label), minibatch, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    TdtAlignParams p = make_params(label_lengths, input_lengths, durations, num_durations, minibatch, workspace, options);
    p.token_frames = token_frames, p.token_durations = token_durations, p.token_logp = token_logp, p.scores = scores;
    return from_hip(launch_tdtalign_path(p, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_tdt_align(const float *acts, const int *flat_labels, const int *label_lengths, const int *input_lengths,
                                    int alphabet_size, const int *durations, int num_durations, float sigma, int minibatch,
                                    int *token_frames, int *token_durations, float *token_logp, float *scores, void *workspace,
                                    rnntOptions options) {
    // everything both halves check, before the first half enqueues anything
    if (!(sigma >= 0.f) || !isfinite(sigma)) return RNNT_STATUS_INVALID_VALUE;
    if (!acts || !aligned4(acts) || !flat_labels || !aligned4(flat_labels)) return RNNT_STATUS_INVALID_VALUE;
    if (!outputs_ok(token_frames, token_durations, token_logp, scores)) return RNNT_STATUS_INVALID_VALUE;
    rnntStatus_t st = check_common(label_lengths, input_lengths, durations, num_durations, workspace, alphabet_size, minibatch, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    st = compute_rnnt_tdt_align_cells(acts, options.maxT, 0, flat_labels, label_lengths, input_lengths, alphabet_size, durations,
                                      num_durations, sigma, minibatch, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return compute_rnnt_tdt_align_path(token_frames, token_durations, token_logp, scores, label_lengths, input_lengths, durations,
                                       num_durations, minibatch, workspace, options);
}

}  // extern "C"
