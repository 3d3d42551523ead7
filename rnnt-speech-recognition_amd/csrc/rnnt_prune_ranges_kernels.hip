// rnnt_prune_ranges_kernels.hip -- where each frame's band of S symbols begins, from the occupancies of the first pass
// (include/rnnt_prune_ranges.h has the rule).
//
//   prune_ranges_window_kernel   step 1.  A wavefront owns one LIVE frame (b, t), t < T_b; the others leave at once.  Lane l takes
//                                the windows s0 = l, l + 64, ... <= hi: adjacent lanes read adjacent addresses, each element is
//                                read S times, from L1 / L2 after the first.  Every lane adds its window's S terms in float64 in
//                                increasing s and keeps (best, s0) with a strict >, from (-inf, 0); the wavefront then reduces the
//                                pairs by "the larger sum, on equal sums the lower s0" -- a total order, so the butterfly's shape
//                                does not matter -- and lane 0 stores raw[b, t] into s_begin.  No window reaches past L_b.
//   prune_ranges_scan_kernel     steps 2 - 5 in place on s_begin: a wavefront per utterance, lane l owns the frames t = l mod 64.
//                                Forwards over chunks of 64 frames: the two fixed ends, an inclusive prefix maximum by shuffles and
//                                a carried value.  Backwards: step 4 in its closed form, sb[t] = max over k >= t of
//                                sb[k] - (k - t)(S - 1), as a suffix maximum of sb[k] - (k - base)(S - 1) inside the chunk and a
//                                carried value from the chunks behind it; then the fill of the frames t >= T_b.  A lane reads back
//                                only what it stored itself, so the passes need no fence between them.
//
// No atomics, no workspace, no LDS: two calls give the same bits and an utterance's result does not depend on its batch.
#include "rnnt_prune_ranges.h"

#include <math.h>

namespace rnnt {

struct PruneRangesLens {
    int Tb, hi;
};

// T_b clamped into [1, maxT], L_b into [0, maxU - 1]; hi = max(0, L_b + 1 - S)
__device__ __forceinline__ PruneRangesLens prune_ranges_lens(const PruneRangesParams &p, const int b) {
    PruneRangesLens m;
    m.Tb = min(max(p.input_lengths[b], 1), p.T);
    const int Lb = min(max(p.label_lengths[b], 0), p.U - 1);
    m.hi = max(0, Lb + 1 - p.S);
    return m;
}

// ---------------------------------------------------------------------------------------------
// Step 1: wavefront r of the grid owns frame r = b T + t.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) prune_ranges_window_kernel(const PruneRangesParams p) {
    const int lane = threadIdx.x & 63;
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= (uint32_t)p.B * (uint32_t)p.T) return;
    const int b = (int)(r / (uint32_t)p.T), t = (int)(r - (uint32_t)b * (uint32_t)p.T);
    const PruneRangesLens m = prune_ranges_lens(p, b);
    if (t >= m.Tb) return;  // padded: not read, and the scan pass writes s_begin there
    double best = -INFINITY;
    int at = 0;
    if (m.hi > 0) {  // (hi = 0: the answer is 0 and nothing is read)
        const float *row = p.occupancy + (size_t)r * (size_t)p.U;
        for (int s0 = lane; s0 <= m.hi; s0 += 64) {  // s0 + S - 1 <= hi + S - 1 = L_b
            double w = (double)row[s0];
            for (int k = 1; k < p.S; ++k) w += (double)row[s0 + k];
            if (w > best) best = w, at = s0;  // (NaN > best is false: a NaN sum never wins)
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ob = __shfl_xor(best, d);
        const int oa = __shfl_xor(at, d);
        if (ob > best || (ob == best && oa < at)) best = ob, at = oa;
    }
    if (lane == 0) p.s_begin[r] = at;
}

// ---------------------------------------------------------------------------------------------
// Steps 2 - 5: workgroup b (one wavefront) owns utterance b.
// ---------------------------------------------------------------------------------------------
constexpr int kPruneRangesDead = -(1 << 30);  // a frame t >= T_b in the suffix maximum: below every candidate, far from overflow

__global__ void __launch_bounds__(64) prune_ranges_scan_kernel(const PruneRangesParams p) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const PruneRangesLens m = prune_ranges_lens(p, b);
    const int Tb = m.Tb, hi = m.hi, step = p.S - 1;
    int *sb = p.s_begin + (size_t)b * (size_t)p.T;
    // steps 2 and 3: raw[0] = 0, then raw[T_b - 1] = hi; the running maximum (every value is >= 0: the carry starts there)
    int carry = 0;
    for (int base = 0; base < Tb; base += 64) {
        const int t = base + lane;
        int v = 0;
        if (t < Tb) {
            v = sb[t];
            if (t == 0) v = 0;
            if (t == Tb - 1) v = hi;
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(v, d);
            if (lane >= d) v = max(v, o);
        }
        v = max(v, carry);
        carry = __shfl(v, 63);
        if (t < Tb) sb[t] = v;
    }
    // step 4 and the fill of step 5.  c: max over the frames k behind this chunk of sb[k] - (k - next)(S - 1), `next` the first
    // frame behind the chunk.  A negative candidate never wins (sb >= 0), so c is kept at -1 or above: nothing grows with T.
    int c = -1;
    for (int base = ((p.T - 1) / 64) * 64; base >= 0; base -= 64) {
        const int t = base + lane;
        const bool live = t < Tb;
        const int v = live ? sb[t] : 0;
        int w = live ? v - lane * step : kPruneRangesDead;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_down(w, d);
            if (lane + d < 64) w = max(w, o);
        }
        w = max(w, c - 64 * step);
        c = max(__shfl(w, 0), -1);
        if (t < p.T) {
            if (!live)
                sb[t] = hi;
            else if (t >= 1)  // (t = T_b - 1: the maximum is its own term; t = 0 stays 0)
                sb[t] = max(v, w + lane * step);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Launchers.  Both grids are one-dimensional; the entry point has checked that B T U < 2^31.
// ---------------------------------------------------------------------------------------------
hipError_t launch_prune_ranges_windows(const PruneRangesParams &p, hipStream_t s) {
    const uint32_t frames = (uint32_t)p.B * (uint32_t)p.T;
    hipLaunchKernelGGL(prune_ranges_window_kernel, dim3((frames + 3) / 4), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_prune_ranges_scan(const PruneRangesParams &p, hipStream_t s) {
    hipLaunchKernelGGL(prune_ranges_scan_kernel, dim3((uint32_t)p.B), dim3(64), 0, s, p);
    return hipGetLastError();
}

}  // namespace rnnt
