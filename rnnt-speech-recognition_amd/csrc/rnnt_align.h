// rnnt_align.h -- forced alignment (include/rnnt.h, "Forced alignment"): workspace layout and launchers of align_kernels.hip.
//
// Workspace, per utterance b:
//   cells  float2 [B][T][Up]   {lpb, lpl} of lattice cell (t, u) at row (t + u) mod T, column u: the cells of anti-diagonal
//                              n = t + u are CONTIGUOUS (row n mod T), and the array is no larger than the lattice itself
//                              (for a fixed column, t -> (t + u) mod T is a bijection of [0, T)).  Row stride Up = the sweep's
//                              threads x columns per thread, so a thread's K cells are one aligned 8K-byte piece.
//   bits   u32 [B][NB][Up]     back-pointers: bit (n mod 32) of word [n / 32][u] is set when cell (n - u, u) was reached by its
//                              label arrival, from (n - u, u - 1).  NB = blocks of 32 diagonals.
#pragma once
#include "rnnt_common.h"

namespace rnnt {

struct AlignLayout {
    size_t cells, bits, total;
    int threads, K, Up, NB;
};

// Columns per thread of the wide sweep (1024 threads, U > 1024): 2 ... 8.
inline int align_wide_K(int U) {
    const int k = (U + 1023) / 1024;
    const int avail[] = {2, 3, 4, 6, 8};
    for (int a : avail)
        if (k <= a) return a;
    return 0;
}

// The workspace of a lattice whose back-pointers take NB blocks of 32 sweep steps: the standard aligner here, the modified one in
// rnnt_modalign.h.  The sweep geometry (threads, K, Up) depends on U alone and is the same for both.
inline AlignLayout make_align_layout_nb(int T, int U, int B, int NB) {
    AlignLayout w;
    w.threads = sweep_K(U) ? 64 : 1024;
    w.K = sweep_K(U) ? sweep_K(U) : align_wide_K(U);
    w.Up = w.threads * w.K;
    w.NB = NB;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    w.cells = take((size_t)B * T * w.Up * 2 * sizeof(float));
    w.bits = take((size_t)B * w.NB * w.Up * sizeof(uint32_t));
    w.total = off;
    return w;
}

inline AlignLayout make_align_layout(int T, int U, int B) {
    return make_align_layout_nb(T, U, B, (T + U - 2) / 32 + 1);  // diagonals 0 ... T + U - 2
}

// The kernel argument of the standard and the modified aligner (the field order is the argument's layout).
struct AlignParams {
    const float *acts;  // the slab [B][S][U][V] (cell pass only)
    const int *labels;  // [B][U-1]
    const int *label_lengths;
    const int *input_lengths;
    float2 *cells;  // {lpb, lpl}: wrapped skew (standard) or row-major [t][u] (modified)
    uint32_t *bits;
    int *token_frames;  // [B][U-1]
    float *token_logp;  // [B][U-1]
    float *scores;      // [B]
    int B, T, U, V, blank;
    int S, t0;  // slab frames, first frame of the slab
    int Up, NB;
    FastDiv divU, divS;
};

hipError_t launch_align_cells(const AlignParams &p, hipStream_t s);
hipError_t launch_align_path(const AlignParams &p, hipStream_t s);

}  // namespace rnnt
