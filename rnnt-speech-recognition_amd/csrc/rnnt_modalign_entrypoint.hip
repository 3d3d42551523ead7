// rnnt_modalign_entrypoint.hip -- the extern "C" boundary of libwarprnnt_modalign.so (declared in include/rnnt_modified_align.h):
// forced alignment on the modified (one symbol per frame) lattice.  The other libraries and their headers stay as they are.
// build.py links this translation unit with rnnt_modalign_kernels.hip alone, and rnnt_modalign.map keeps everything but the four
// entry points local.  Argument validation follows compute_rnnt_align's: everything is checked before anything is enqueued,
// nothing is allocated, everything is enqueued on the caller's stream.
#include "../../include/rnnt_modified_align.h"
#include "rnnt_modalign.h"
#include "rnnt_host.h"

using namespace rnnt;

// the shape limits of the op (include/rnnt.h): maxU <= 8192, minibatch * maxT * maxU < 2^31
static bool shape_ok(int maxT, int maxU, int minibatch) {
    if (maxT <= 0 || maxU <= 0 || maxU > kMaxU || minibatch <= 0) return false;
    return (long long)minibatch * maxT * maxU < (1ll << 31);
}

static rnntStatus_t check_common(const void *labels, const void *ll, const void *il, const void *ws, int V, int B,
                                 const rnntOptions &o) {
    if (!labels || !ll || !il || !ws) return RNNT_STATUS_INVALID_VALUE;
    if (!aligned4(labels) || !aligned4(ll) || !aligned4(il)) return RNNT_STATUS_INVALID_VALUE;
    if (o.loc != RNNT_GPU || !o.batch_first) return RNNT_STATUS_INVALID_VALUE;  // device-only library: no CPU fallback
    if (V < 2 || o.blank_label < 0 || o.blank_label >= V) return RNNT_STATUS_INVALID_VALUE;
    if (!shape_ok(o.maxT, o.maxU, B)) return RNNT_STATUS_INVALID_VALUE;
    if (((uintptr_t)ws & 255) != 0) return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}

static AlignParams make_params(const int *labels, const int *ll, const int *il, int V, int B, void *ws, const rnntOptions &o) {
    const AlignLayout w = make_modalign_layout(o.maxT, o.maxU, B);
    AlignParams p{};
    p.labels = labels, p.label_lengths = ll, p.input_lengths = il;
    p.cells = (float2 *)((char *)ws + w.cells);
    p.bits = (uint32_t *)((char *)ws + w.bits);
    p.B = B, p.T = o.maxT, p.U = o.maxU, p.V = V, p.blank = o.blank_label;
    p.Up = w.Up, p.NB = w.NB;
    p.divU = make_fastdiv((uint32_t)o.maxU);
    return p;
}

extern "C" {

rnntStatus_t get_rnnt_modified_align_workspace_size(int maxT, int maxU, int minibatch, size_t *size_bytes) {
    if (!size_bytes || !shape_ok(maxT, maxU, minibatch)) return RNNT_STATUS_INVALID_VALUE;
    *size_bytes = make_modalign_layout(maxT, maxU, minibatch).total;
    return RNNT_STATUS_SUCCESS;
}

rnntStatus_t compute_rnnt_modified_align_cells(const float *acts_slab, int slab_frames, int frame_offset, const int *flat_labels,
                                               const int *label_lengths, const int *input_lengths, int alphabet_size,
                                               int minibatch, void *workspace, rnntOptions options) {
    if (!acts_slab || !aligned4(acts_slab)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_common(flat_labels, label_lengths, input_lengths, workspace, alphabet_size, minibatch, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (slab_frames < 1 || frame_offset < 0 || (long long)frame_offset + slab_frames > options.maxT) return RNNT_STATUS_INVALID_VALUE;
    AlignParams p = make_params(flat_labels, label_lengths, input_lengths, alphabet_size, minibatch, workspace, options);
    p.acts = acts_slab, p.S = slab_frames, p.t0 = frame_offset;
    p.divS = make_fastdiv((uint32_t)slab_frames);
    return from_hip(launch_modalign_cells(p, (hipStream_t)options.stream));
}

// alphabet_size does not enter the sweep; the entry point takes none
rnntStatus_t compute_rnnt_modified_align_path(int *token_frames, float *token_logp, float *scores, const int *label_lengths,
                                              const int *input_lengths, int minibatch, void *workspace, rnntOptions options) {
    if (!token_frames || !token_logp || !scores || !aligned4(token_frames) || !aligned4(token_logp) || !aligned4(scores))
        return RNNT_STATUS_INVALID_VALUE;
    // (the blank's range was checked against the vocabulary by the _cells calls that filled the workspace)
    const rnntStatus_t st =
        check_common(label_lengths, label_lengths, input_lengths, workspace, vocab_holding(options.blank_label), minibatch, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    AlignParams p = make_params(nullptr, label_lengths, input_lengths, 0, minibatch, workspace, options);
    p.token_frames = token_frames, p.token_logp = token_logp, p.scores = scores;
    return from_hip(launch_modalign_path(p, (hipStream_t)options.stream));
}

rnntStatus_t compute_rnnt_modified_align(const float *acts, const int *flat_labels, const int *label_lengths,
                                         const int *input_lengths, int alphabet_size, int minibatch, int *token_frames,
                                         float *token_logp, float *scores, void *workspace, rnntOptions options) {
    if (!acts || !aligned4(acts)) return RNNT_STATUS_INVALID_VALUE;
    if (!token_frames || !token_logp || !scores || !aligned4(token_frames) || !aligned4(token_logp) || !aligned4(scores))
        return RNNT_STATUS_INVALID_VALUE;
    rnntStatus_t st = check_common(flat_labels, label_lengths, input_lengths, workspace, alphabet_size, minibatch, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    st = compute_rnnt_modified_align_cells(acts, options.maxT, 0, flat_labels, label_lengths, input_lengths, alphabet_size,
                                           minibatch, workspace, options);
    if (st != RNNT_STATUS_SUCCESS) return st;
    return compute_rnnt_modified_align_path(token_frames, token_logp, scores, label_lengths, input_lengths, minibatch, workspace,
                                            options);
}

}  // extern "C"
