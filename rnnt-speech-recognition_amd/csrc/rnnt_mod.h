// rnnt_mod.h -- the modified (one symbol per frame) topology of the transducer loss (include/rnnt_modified.h):
// workspace layout and launchers of rnnt_mod_kernels.hip.
//
// Lattice nodes (t, u), 0 <= t <= T_b, 0 <= u <= L_b; every edge advances the frame:
//   alpha(t,u) = logaddexp(alpha(t-1,u) + lpb(t-1,u), alpha(t-1,u-1) + lpl(t-1,u-1)),  ln P = alpha(T_b, L_b)
//   beta(t,u)  = logaddexp(lpb(t,u) + beta(t+1,u),    lpl(t,u) + beta(t+1,u+1)),       beta(T_b, L_b) = 0
// Row t depends on row t -+ 1 only: the sweeps take T_b serial steps with every column in flight.
//
// Workspace, Up = the sweep's threads x columns per thread (the aligner's geometry, rnnt_align.h):
//   lp     float2 [B][T][Up]     {lpb, lpl} of the live cells inside the band u <= t, L_b - u <= T_b - t; nothing else is written
//   lse    f32    [B][T][U]      the natural-log softmax denominator of the same cells
//   alpha  f64    [B][T][Up]     rows 0 ... T_b - 1, every column: -inf outside the band
//   beta   f64    [B][T+1][Up]   rows 0 ... T_b, every column: -inf outside the band
//   lnP    f64    [B]            alpha(T_b, L_b); -inf for an infeasible utterance (L_b > T_b), NaN for out-of-range lengths
// Everything a kernel reads was written by the kernel in front of it: the workspace may hold anything on entry.
#pragma once
#include "rnnt_align.h"

namespace rnnt {

struct ModLayout {
    size_t lp, lse, alpha, beta, lnP, total;
    int Up;
};

inline ModLayout make_mod_layout(int T, int U, int B) {
    ModLayout w;
    const AlignLayout a = make_align_layout(T, U, B);
    w.Up = a.Up;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    w.lp = take((size_t)B * T * w.Up * 2 * sizeof(float));
    w.lse = take((size_t)B * T * U * sizeof(float));
    w.alpha = take((size_t)B * T * w.Up * sizeof(double));
    w.beta = take((size_t)B * (T + 1) * w.Up * sizeof(double));
    w.lnP = take((size_t)B * sizeof(double));
    w.total = off;
    return w;
}

struct ModParams {
    const float *acts;  // [B][T][U][V]
    float *grads;       // [B][T][U][V] (gradient pass only)
    const int *labels;  // [B][U-1]
    const int *label_lengths;
    const int *input_lengths;
    const float *cost_scale;  // nullable
    float *costs;             // [B] (sweeps only)
    float2 *lp;
    float *lse;
    double *alpha;
    double *beta;
    double *lnP;
    int B, T, U, V, blank;
    int Up;
    float fe_lambda;
    FastDiv divU, divT;
};

hipError_t launch_mod_cells(const ModParams &p, hipStream_t s);
hipError_t launch_mod_sweeps(const ModParams &p, hipStream_t s);
hipError_t launch_mod_grad(const ModParams &p, hipStream_t s);

}  // namespace rnnt
