// rnnt_ctc.h -- the CTC loss and the greedy CTC decoder (include/rnnt_ctc.h): workspace layout, tier constants and launchers of
// rnnt_ctc_kernels.hip.
//
// States s = 0 ... 2 L_b; a sweep thread owns label POSITIONS, K of them.  Position k of the alpha sweep is the pair
// (blank state 2k, label state 2k + 1 = y_k); position j of the beta sweep is the mirrored pair (blank state 2j, label state
// 2j - 1 = y_{j-1}).  With that ownership a step needs ONE value from the neighbouring position, its label state on the row before:
//   alpha:  from = alpha(t-1, 2k-1)     b' = lpb + logadd(b, from)      l' = lp(y_k)     + logadd3(l, b, skip_k ? from : -inf)
//   beta:   from = beta(t+1, 2j+1)      b' = lpb + logadd(b, from)      l' = lp(y_{j-1}) + logadd3(l, b, skip_j ? from : -inf)
// skip_k = 1 <= k < L_b and y_k != y_{k-1}: the same bit serves both directions.
//
// Workspace, Up = the sweep's threads x positions per thread:
//   lpa    float2 [B][T][Up]   {lp(t, blank), lp(t, y_k)} at column k <= L_b of the live frames (.y only for k < L_b); nothing else is written
//   lpb    float2 [B][T][Up]   {lp(t, blank), lp(t, y_{j-1})} at column j <= L_b (.y only for j >= 1): the beta sweep's aligned copy
//   lse    f32    [B][T]       the natural-log softmax denominator of the live frames
//   alpha  double2 [B][T][Up]  {alpha(t, 2k), alpha(t, 2k+1)}, rows 0 ... T_b - 1, every column: -inf outside the lattice
//   beta   double2 [B][T][Up]  {beta(t, 2j), beta(t, 2j-1)}, the same
//   lnP    f64    [B]          -inf for an utterance without a path, NaN for an invalid one
//   meta   i32    [B][Up]      per position k < L_b: kCtcSkip, kCtcFirst (no earlier position holds y_k), and in the bits from
//                              kCtcNextShift up the next position that holds y_k, plus one (0: none)
//   lab    i32    [B][Up]      the labels clamped into [0, V)
//   flags  i32    [B]          1: out-of-range lengths or a label equal to the blank
// Everything a kernel reads was written by the kernel in front of it: the workspace may hold anything on entry.
#pragma once
#include "rnnt_common.h"

namespace rnnt {

// The sweep tiers by positions U = maxU (tests/test_ctc_gpu.py reads these lines): one wavefront with K positions per thread up to
// kCtcWaveThreads * 16 positions, one workgroup of kCtcWideThreads threads beyond.
constexpr int kCtcWaveThreads = 64;
constexpr int kCtcWideThreads = 1024;
constexpr int kCtcWaveK[] = {1, 2, 3, 4, 6, 8, 12, 16};
constexpr int kCtcWideK[] = {2, 3, 4, 6, 8};
constexpr int kCtcRowVec = 4;        // floats per lane and load of the row pass on 16-byte-aligned rows (else 1)
constexpr int kCtcGradTile = 4096;   // columns of the softmax row the gradient pass stages in LDS at a time
constexpr int kCtcGradThreads = 256;
constexpr int kCtcGreedyChunk = 64;  // frames the greedy decoder compacts at a time (one ballot)

constexpr int kCtcSkip = 1, kCtcFirst = 2, kCtcNextShift = 2;

struct CtcTier {
    int threads, K;
};
inline CtcTier ctc_tier(int U) {
    for (int k : kCtcWaveK)
        if (U <= kCtcWaveThreads * k) return {kCtcWaveThreads, k};
    for (int k : kCtcWideK)
        if (U <= kCtcWideThreads * k) return {kCtcWideThreads, k};
    return {0, 0};
}

struct CtcLayout {
    size_t lpa, lpb, lse, alpha, beta, lnP, meta, lab, flags, total;
    int Up;
};

inline CtcLayout make_ctc_layout(int T, int U, int B) {
    CtcLayout w;
    const CtcTier tier = ctc_tier(U);
    w.Up = tier.threads * tier.K;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    w.lpa = take((size_t)B * T * w.Up * 2 * sizeof(float));
    w.lpb = take((size_t)B * T * w.Up * 2 * sizeof(float));
    w.lse = take((size_t)B * T * sizeof(float));
    w.alpha = take((size_t)B * T * w.Up * 2 * sizeof(double));
    w.beta = take((size_t)B * T * w.Up * 2 * sizeof(double));
    w.lnP = take((size_t)B * sizeof(double));
    w.meta = take((size_t)B * w.Up * sizeof(int));
    w.lab = take((size_t)B * w.Up * sizeof(int));
    w.flags = take((size_t)B * sizeof(int));
    w.total = off;
    return w;
}

struct CtcParams {
    const float *acts;  // [B][T][V]
    float *grads;       // [B][T][V] (gradient pass only)
    const int *labels;  // [B][U-1]
    const int *label_lengths;
    const int *input_lengths;
    const float *cost_scale;  // nullable
    float *costs;             // [B] (sweeps only)
    float2 *lpa, *lpb;
    float *lse;
    double2 *alpha, *beta;
    double *lnP;
    int *meta, *lab, *flags;
    int B, T, U, V, blank;
    int Up;
};

struct CtcGreedyParams {
    const float *acts;  // [B][T][V]
    const int *input_lengths;
    int *tokens, *token_frames, *lengths;  // token_frames nullable
    int B, T, V, blank;
};

hipError_t launch_ctc_prepare(const CtcParams &p, hipStream_t s);
hipError_t launch_ctc_rows(const CtcParams &p, hipStream_t s);
hipError_t launch_ctc_sweeps(const CtcParams &p, hipStream_t s);
hipError_t launch_ctc_grad(const CtcParams &p, hipStream_t s);
hipError_t launch_ctc_greedy(const CtcGreedyParams &p, hipStream_t s);

}  // namespace rnnt
