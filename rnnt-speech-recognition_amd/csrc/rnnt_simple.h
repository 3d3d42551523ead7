// rnnt_simple.h -- the SIMPLE (additive joiner) transducer loss (include/rnnt_simple.h): workspace layout and launchers of
// rnnt_simple_kernels.hip.  logit(t, u, v) = am[t, v] + lm[u, v]; the [B, T, U, V] tensor is never formed.
//
// One sweep kernel serves both lattices through a SKEWED step index: lattice cell (t, u) lives in row n = t + skew u of the
// lattice arrays, skew = 1 on the standard lattice (n is the anti-diagonal), 0 on the modified one (n is the frame).  In both,
// row n + 1 depends on row n alone: the blank edge of (t, u) ends in lane u of row n + 1, its label edge in lane u + 1 of row
// n + 1.  Nodes (t, u) are VALID iff 0 <= t < T_b and u <= L_b, plus the end node (T_b, L_b): the standard lattice's final blank
// is the blank edge of (T_b - 1, L_b) into it, and nothing else reaches it there (cell (T_b, L_b - 1) is not valid); on the
// modified lattice the label edge of (T_b - 1, L_b - 1) reaches it too.  ln P = alpha(end node) in both.
//
// Workspace, NR = maxT + maxU - 1 rows, Up = the sweep's threads x columns per thread; a function of
// (maxT, maxU, minibatch) alone:
//   lp     float2 [B][NR][Up]    {lpb, lpl} of the present cells at their skewed place; nothing else is written
//   alpha  f64    [B][NR][Up]    rows 0 ... nsteps - 1, every column: -inf on nodes that are not valid
//   beta   f64    [B][NR+1][Up]  rows 0 ... nsteps, every column likewise (nsteps = T_b + skew L_b)
//   Z      f32    [B][T][U]      ln sum_v exp(am + lm) of the present cells
//   e      float2 [B][T][U]      {e_b, e_l} of EVERY cell (zeros on absent ones; NaN on the clamped lattice of a bad utterance)
//   Za     f32    [B][T]         ln sum_v exp(am[t]) of the rows t < T_b;   Zl f32 [B][U] likewise of the rows u <= L_b
//   lnP    f64    [B]            -inf without a path (modified, L_b > T_b), NaN for out-of-range lengths
// Everything a kernel reads was written by a kernel in front of it: the workspace may hold anything on entry.
#pragma once
#include "rnnt_align.h"

namespace rnnt {

constexpr int kSimpleMaxU = 8192;

struct SimpleLayout {
    size_t lp, alpha, beta, Z, e, Za, Zl, lnP, total;
    int Up, NR;
};

inline SimpleLayout make_simple_layout(int T, int U, int B) {
    SimpleLayout w;
    w.Up = sweep_K(U) ? 64 * sweep_K(U) : 1024 * align_wide_K(U);
    w.NR = T + U - 1;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    w.lp = take((size_t)B * w.NR * w.Up * 2 * sizeof(float));
    w.alpha = take((size_t)B * w.NR * w.Up * sizeof(double));
    w.beta = take((size_t)B * (w.NR + 1) * w.Up * sizeof(double));
    w.Z = take((size_t)B * T * U * sizeof(float));
    w.e = take((size_t)B * T * U * 2 * sizeof(float));
    w.Za = take((size_t)B * T * sizeof(float));
    w.Zl = take((size_t)B * U * sizeof(float));
    w.lnP = take((size_t)B * sizeof(double));
    w.total = off;
    return w;
}

struct SimpleParams {
    const float *am;  // [B][T][V]
    const float *lm;  // [B][U][V]
    float *grad_am;   // [B][T][V] (gradient passes only)
    float *grad_lm;   // [B][U][V]
    float *occupancy;  // [B][T][U], nullable
    const int *labels;  // [B][U-1]
    const int *label_lengths;
    const int *input_lengths;
    const float *cost_scale;  // nullable
    float *costs;             // [B] (sweeps only)
    float2 *lp;
    double *alpha;
    double *beta;
    float *Z;
    float2 *e;
    float *Za;
    float *Zl;
    double *lnP;
    int B, T, U, V, blank;
    int Up, NR;
    int skew;  // 1: standard, 0: modified
    float a_scale, l_scale, w_scale;  // am_only_scale, lm_only_scale, 1 - a - l
};

hipError_t launch_simple_rows(const SimpleParams &p, hipStream_t s);
hipError_t launch_simple_cells(const SimpleParams &p, hipStream_t s);
hipError_t launch_simple_sweeps(const SimpleParams &p, hipStream_t s);
hipError_t launch_simple_occupancy(const SimpleParams &p, hipStream_t s);
hipError_t launch_simple_grads(const SimpleParams &p, hipStream_t s);

}  // namespace rnnt
