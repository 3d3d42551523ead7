// rnnt_tdt.h -- the token-and-duration (TDT) transducer loss (include/rnnt_tdt.h): workspace layout and launchers of
// rnnt_tdt_kernels.hip.
//
// Lattice nodes (t, u), 0 <= t < T_b, 0 <= u <= L_b, and the terminal (T_b, L_b).  From (t, u), for every duration d_i:
//   blank edge to (t + d_i, u)      wb_i = lp(t,u,blank) - sigma + ld(t,u,i)   iff d_i > 0 and the target is a node
//   label edge to (t + d_i, u + 1)  wl_i = lp(t,u,y_u)  - sigma + ld(t,u,i)   iff u < L_b and t + d_i < T_b
// alpha pulls over incoming edges, beta over outgoing ones; ln P = alpha(T_b, L_b).
//
// Every per-node array is SKEWED: node (t, u) lives at row n = t + u, column u, so that the nodes of one sweep step (one n, lanes =
// columns) are contiguous.  An edge of duration d joins row n to row n + d (blank, same column) or n + d + 1 (label, next column):
// a row depends on the dmax + 1 rows before it (alpha) or after it (beta).
//
// Workspace, N = T + U rows, Up = U rounded up to 64 (the sweep's threads), D2 = 2 D:
//   w      f32 [B][D2][N][Up]   the edge weights of the live cells: plane i = wb_i, plane D + i = wl_i (whether or not the edge
//                               exists); nothing else is written.  One plane per edge kind: the alpha sweep reads plane i of row
//                               n - d_i (the SOURCE cell's weight), the beta sweep plane i of its own row, both along the lanes.
//   lse    float2 [B][T][U]     {token, duration} natural-log softmax denominators of the live cells (cell order: the gradient pass)
//   alpha  f64 [B][N][Up]       rows 0 ... T_b + L_b, every column: -inf where there is no node or no path from (0, 0)
//   beta   f64 [B][N][Up]       the same rows: -inf where there is no node or no path to the terminal
//   lnP    f64 [B]              alpha(T_b, L_b); -inf for an utterance without a path, NaN for out-of-range lengths
// Everything a kernel reads was written by the kernel in front of it: the workspace may hold anything on entry.
#pragma once
#include "rnnt_common.h"
#include "tdt_host.h"

namespace rnnt {

constexpr int kTdtMaxU = 1024;      // one lattice column per thread of the sweep
constexpr int kTdtMaxD = 8;         // durations per set
constexpr int kTdtMaxDuration = 8;  // the largest duration: the sweep's ring holds kTdtMaxDuration + 2 rows
static_assert(kTdtMaxD == kTdtHostMaxD && kTdtMaxDuration == kTdtHostMaxDuration, "tdt_host.h holds the limits the boundary checks");

struct TdtLayout {
    size_t w, lse, alpha, beta, lnP, total;
    int Up, N;
};

inline TdtLayout make_tdt_layout(int T, int U, int B, int D) {
    TdtLayout l;
    l.Up = (int)align_up((size_t)U, 64);
    l.N = T + U;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    l.w = take((size_t)B * 2 * D * l.N * l.Up * sizeof(float));
    l.lse = take((size_t)B * T * U * 2 * sizeof(float));
    l.alpha = take((size_t)B * l.N * l.Up * sizeof(double));
    l.beta = take((size_t)B * l.N * l.Up * sizeof(double));
    l.lnP = take((size_t)B * sizeof(double));
    l.total = off;
    return l;
}

struct TdtParams {
    const float *acts;  // [B][T][U][V + D]
    float *grads;       // [B][T][U][V + D] (gradient pass only)
    const int *labels;  // [B][U-1]
    const int *label_lengths;
    const int *input_lengths;
    const float *cost_scale;  // nullable
    float *costs;             // [B] (sweeps only)
    float *w;
    float2 *lse;
    double *alpha;
    double *beta;
    double *lnP;
    int B, T, U, V, D, blank;
    int Up, N;
    int dur[kTdtMaxD];  // strictly increasing; entries past D are not read
    float sigma;
    FastDiv divU, divT;
};

hipError_t launch_tdt_cells(const TdtParams &p, hipStream_t s);
hipError_t launch_tdt_sweeps(const TdtParams &p, hipStream_t s);
hipError_t launch_tdt_grad(const TdtParams &p, hipStream_t s);

}  // namespace rnnt
