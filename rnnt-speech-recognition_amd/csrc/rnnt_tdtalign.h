// rnnt_tdtalign.h -- forced alignment on the token-and-duration (TDT) lattice (include/rnnt_tdt_align.h): workspace layout and
// launchers of rnnt_tdtalign_kernels.hip.
//
// Lattice nodes (t, u), 0 <= t < T_b, 0 <= u <= L_b, and the terminal (T_b, L_b).  From (t, u), for every duration d_i:
//   blank edge to (t + d_i, u)      wb_i = lp(t,u,blank) - sigma + ld(t,u,i)   iff d_i > 0 and the target is a node
//   label edge to (t + d_i, u + 1)  wl_i = lp(t,u,y_u)  - sigma + ld(t,u,i)   iff u < L_b and t + d_i < T_b
// v pulls the maximum over incoming edges; score = v(T_b, L_b).
//
// Every per-node array is SKEWED as in rnnt_tdt.h: node (t, u) lives at row n = t + u, column u.  An edge of duration d joins row n
// to row n + d (blank, same column) or n + d + 1 (label, next column): a row depends on the dmax + 1 rows before it.
//
// Workspace, N = T + U rows, Up = U rounded up to 64 (the sweep's threads):
//   sigma  f32 [1]               what the cell passes were given (the back-trace adds it back for token_logp)
//   w      f32 [B][2 D][N][Up]   the edge weights of the live cells: plane i = wb_i, plane D + i = wl_i (whether or not the edge
//                                exists); nothing else is written, and the weight of an edge that does not exist is never loaded
//   dec    u8  [B][N][Up]        rows 0 ... T_b + L_b, every column: the decision code 2 i + label of the node there, 0xFF where
//                                nothing arrives.  The sweep writes them before its back-trace reads them.
// Everything a kernel reads was written by the kernel in front of it: the workspace may hold anything on entry.
#pragma once
#include "rnnt_common.h"
#include "tdt_host.h"

namespace rnnt {

constexpr int kTdtAlignMaxU = 1024;      // one lattice column per thread of the sweep
constexpr int kTdtAlignMaxD = 8;         // durations per set
constexpr int kTdtAlignMaxDuration = 8;  // the largest duration: the sweep's ring holds kTdtAlignMaxDuration + 2 rows
static_assert(kTdtAlignMaxD == kTdtHostMaxD && kTdtAlignMaxDuration == kTdtHostMaxDuration, "tdt_host.h holds the limits the boundary checks");

struct TdtAlignLayout {
    size_t sigma, w, dec, total;
    int Up, N;
};

inline TdtAlignLayout make_tdtalign_layout(int T, int U, int B, int D) {
    TdtAlignLayout l;
    l.Up = (int)align_up((size_t)U, 64);
    l.N = T + U;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    l.sigma = take(sizeof(float));
    l.w = take((size_t)B * 2 * D * l.N * l.Up * sizeof(float));
    l.dec = take((size_t)B * l.N * l.Up);
    l.total = off;
    return l;
}

struct TdtAlignParams {
    const float *acts;  // the slab [B][S][U][V + D] (cell pass only)
    const int *labels;  // [B][U-1] (cell pass only)
    const int *label_lengths;
    const int *input_lengths;
    float *sigma_slot;
    float *w;
    uint8_t *dec;
    int *token_frames;     // [B][U-1]
    int *token_durations;  // [B][U-1]
    float *token_logp;     // [B][U-1]
    float *scores;         // [B]
    int B, T, U, V, D, blank;
    int S, t0;  // slab frames, first frame of the slab
    int Up, N;
    int dur[kTdtAlignMaxD];  // strictly increasing; entries past D are not read
    uint32_t dur_packed;      // 4 bits per entry: the back-trace looks a duration up by a run-time index
    float sigma;
    FastDiv divU, divS;
};

hipError_t launch_tdtalign_cells(const TdtAlignParams &p, hipStream_t s);
hipError_t launch_tdtalign_path(const TdtAlignParams &p, hipStream_t s);

}  // namespace rnnt
