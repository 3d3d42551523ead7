// rnnt_pruned.h -- the pruned transducer loss (include/rnnt_pruned.h): workspace layout and launchers of rnnt_pruned_kernels.hip.
// Self-contained: nothing of the other libraries' sources is included.
//
// The tensor has B x T x S slots; slot (b, t, s) is lattice cell (t, u), u = sb[b][t] + s, PRESENT iff t < T_b, 0 <= u <= L_b.
//
// Workspace, all [B][T][S], a function of (maxT, s_range, minibatch) alone:
//   lp     float2   {lpb, lpl} of the present cells; nothing else is written (lpl only for u < L_b)
//   lse    f32      the natural-log softmax denominator of the same cells
//   alpha  f64      every slot of the rows t < T_b: -inf for absent cells
//   edge   double2  every slot of the rows t < T_b: {lpb + beta(blank target), lpl + beta(label target)}, the two outgoing edge
//                   terms of the backward recurrence (-inf where the edge or its target is absent; lpb alone on the standard
//                   lattice's final blank).  The gradient pass needs nothing of the neighbouring rows: e_b = exp(alpha + edge.x
//                   - ln P), e_l = exp(alpha + edge.y - ln P).
//   lnP    f64 [B]  -inf for a band that does not connect, NaN for out-of-range lengths
// Everything a kernel reads was written by the kernel in front of it: the workspace may hold anything on entry.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rnnt {

constexpr int kPrunedMaxS = 64;
constexpr int kPrunedMaxU = 8192;

struct PrunedLayout {
    size_t lp, lse, alpha, edge, lnP, total;
};

inline PrunedLayout make_pruned_layout(int T, int S, int B) {
    PrunedLayout w;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = (off + bytes + 255) / 256 * 256;
        return o;
    };
    const size_t n = (size_t)B * T * S;
    w.lp = take(n * 2 * sizeof(float));
    w.lse = take(n * sizeof(float));
    w.alpha = take(n * sizeof(double));
    w.edge = take(n * 2 * sizeof(double));
    w.lnP = take((size_t)B * sizeof(double));
    w.total = off;
    return w;
}

struct PrunedParams {
    const float *acts;  // [B][T][S][V]
    float *grads;       // [B][T][S][V] (gradient pass only)
    const int *s_begin;  // [B][T]
    const int *labels;   // [B][U-1]
    const int *label_lengths;
    const int *input_lengths;
    const float *cost_scale;  // nullable
    float *costs;             // [B] (sweeps only)
    float2 *lp;
    float *lse;
    double *alpha;
    double2 *edge;
    double *lnP;
    int B, T, S, U, V, blank;
    int topology;
    float fe_lambda;
};

hipError_t launch_pruned_cells(const PrunedParams &p, hipStream_t s);
hipError_t launch_pruned_sweeps(const PrunedParams &p, hipStream_t s);
hipError_t launch_pruned_grad(const PrunedParams &p, hipStream_t s);

}  // namespace rnnt
