// align_kernels.hip -- forced alignment: the maximum-probability monotone path through the T x (U+1) lattice the loss sums over
// (include/rnnt.h "Forced alignment").
//
//   align_cells_kernel<L, VEC>   one pass over a slab of logits: log-softmax normaliser per lattice cell (f32, online max / sum,
//                                L lanes per cell), written as {lpb, lpl} on the wrapped-skew grid of rnnt_align.h.  HBM-bound.
//   align_path_kernel<K, G, W>   one workgroup per utterance: max-plus sweep over the anti-diagonals in float64 registers (K lattice
//                                columns per thread; one wavefront up to 1024 columns, 1024 threads beyond), one decision bit per
//                                cell, then the back-trace (wave 0, scalar walk over register-held bit windows) and the outputs.
//
// The normaliser, the cell decomposition, the lane dispatch, the DPP shift, the row loader, the <K, G, W> table and the back-trace
// are those of rnnt_align_parts.h, shared with the modified and the TDT aligner; what is here is this lattice's own: where a cell
// is stored, the diagonal-order step with its masks, the score and the outputs.
//
// Every sum has an order fixed by (V) alone in the cell pass and by the utterance's own cells in the sweep: an utterance's outputs
// do not depend on the batch around it nor on how the frames were cut into slabs.
#include "rnnt_align_parts.h"

namespace rnnt {

// Cell pass (rnnt_align_parts.h): {lpb, lpl} of every cell of the utterance's lattice.
template <int L, bool VEC>
__global__ void __launch_bounds__(256) align_cells_kernel(const AlignParams p) {
    const int j = threadIdx.x % L;
    AlignCell q;
    if (!align_cell_of<L>(p, q)) return;
    const int V = p.V, b = q.b, t = q.t, u = q.u;
    const float *row = p.acts + (size_t)q.c * (size_t)V;
    float m, s;
    align_cell_max_sum<L, VEC>(row, V, j, m, s);
    if (j != 0) return;
    const float lse = m + __logf(s);
    float2 out;
    out.x = row[p.blank] - lse;
    out.y = 0.0f;
    if (u < q.Ub) out.y = row[align_label(p, b, u, V)] - lse;
    int r = t + u;  // wrapped skew: diagonal n = t + u lives in row n mod T
    r = r >= p.T ? r % p.T : r;
    p.cells[((size_t)b * p.T + r) * (size_t)p.Up + u] = out;
}

hipError_t launch_align_cells(const AlignParams &p, hipStream_t s) {
    const bool vec = (p.V % 4 == 0) && (((uintptr_t)p.acts & 15) == 0);
    return dispatch_cell_lanes((p.V + 3) / 4, [&](auto L) {
        constexpr int kL = decltype(L)::value;
        if (vec)
            hipLaunchKernelGGL((align_cells_kernel<kL, true>), dim3(align_cells_grid(p, kL)), dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((align_cells_kernel<kL, false>), dim3(align_cells_grid(p, kL)), dim3(256), 0, s, p);
        return hipGetLastError();
    });
}

// ---------------------------------------------------------------------------------------------
// Sweep + back-trace.  Thread j owns the lattice columns j K ... j K + K - 1.  "Push" form of the recurrence: a cell of diagonal
// n - 1 with value v offers v + lpb to (t + 1, u) -- the same column -- and v + lpl to (t, u + 1) -- the next column --, both on
// diagonal n; only the last column's label offer crosses to the next thread (a whole-wave DPP shift, or LDS + one barrier per
// diagonal in the wide kernel).  The tie rule of include/rnnt.h: the label arrival wins only if STRICTLY greater.
// ---------------------------------------------------------------------------------------------
template <int K, int G, bool WIDE>
__global__ void __launch_bounds__(WIDE ? 1024 : 64) align_path_kernel(const AlignParams p) {
    constexpr int kThreads = WIDE ? 1024 : 64;
    constexpr int kFrames = WIDE ? kMaxU : 1024;
    __shared__ int fr[kFrames];                    // emission frame per token, written by the back-trace
    __shared__ double xch[WIDE ? 2 * 1024 : 2];    // the wide kernel's neighbour exchange, double-buffered by diagonal parity
    const int b = blockIdx.x, tid = threadIdx.x;
    int Tb = p.input_lengths[b], Ub = p.label_lengths[b];
    const bool bad = Tb < 1 || Tb > p.T || Ub < 0 || Ub > p.U - 1;
    Tb = min(max(Tb, 1), p.T);
    Ub = min(max(Ub, 0), p.U - 1);
    const int T = p.T, Up = p.Up;
    const int u0 = tid * K;
    const float2 *cells = p.cells + (size_t)b * T * (size_t)Up;
    uint32_t *bits = p.bits + (size_t)b * p.NB * (size_t)Up;
    const int last = Tb - 1 + Ub;  // the diagonal of the final cell (T_b - 1, U_b)

    double v[K];
    uint32_t w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = (u0 + k == 0) ? 0.0 : -INFINITY;
        w[k] = 0u;
    }

    for (int uu = tid; uu < kFrames; uu += kThreads) fr[uu] = 0;  // (a NaN lattice may leave tokens unvisited: keep reads in bounds)

    int lrow = 0;  // row (= diagonal mod T) of the next diagonal to load
    auto load_block = [&](AlignRow<K>(&buf)[G]) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            align_load_row<K>(buf[g], cells + (size_t)lrow * Up + u0);
            lrow = (lrow + 1 == T) ? 0 : lrow + 1;
        }
    };
    // one diagonal: n = destination diagonal, d = the cells of diagonal n - 1
    auto step = [&](const int n, const AlignRow<K> &d) {
        double a[K], c[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int u = u0 + k;
            const bool src_ok = (unsigned)(n - 1 - u) < (unsigned)Tb && u <= Ub;  // padding / poisoned cells never enter a sum
            a[k] = v[k] + (double)(src_ok ? d.e[k].x : 0.0f);
            c[k] = v[k] + (double)(src_ok ? d.e[k].y : 0.0f);
        }
        double cin;
        if constexpr (WIDE) {
            double *x = xch + (n & 1) * 1024;
            x[tid] = c[K - 1];
            __syncthreads();
            cin = tid ? x[tid - 1] : -INFINITY;
        } else {
            cin = align_from_lower_lane(c[K - 1], -INFINITY);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int u = u0 + k;
            const double from = k ? c[k - 1] : cin;
            const bool dst_ok = (unsigned)(n - u) < (unsigned)Tb && u <= Ub;
            const bool lab = from > a[k];  // strictly greater: an exact tie takes the blank arrival
            v[k] = dst_ok ? (lab ? from : a[k]) : -INFINITY;
            w[k] |= (uint32_t)(lab && dst_ok) << (n & 31);
        }
        if ((n & 31) == 31 || n == last) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                bits[(size_t)(n >> 5) * Up + u0 + k] = w[k];
                w[k] = 0u;
            }
        }
    };

    AlignRow<K> bufA[G], bufB[G];
    load_block(bufA);
    for (int s0 = 0; s0 < last; s0 += 2 * G) {
        load_block(bufB);
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (s0 + g + 1 <= last) step(s0 + g + 1, bufA[g]);
        load_block(bufA);
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (s0 + G + g + 1 <= last) step(s0 + G + g + 1, bufB[g]);
    }

    // the score: the final cell's value plus its blank
    {
        double vf = -INFINITY;
        bool mine = false;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (u0 + k == Ub) vf = v[k], mine = true;
        if (mine) {
            const float lpb = cells[(size_t)(last % T) * Up + Ub].x;
            p.scores[b] = bad ? __int_as_float(0x7fc00000) : (float)(vf + (double)lpb);
        }
    }
    __threadfence();  // the decision words are read back by other lanes below
    __syncthreads();

    // Back-trace (rnnt_align_parts.h): T_b + U_b - 1 dependent steps on wave 0.  A set bit of diagonal n in column u: token u - 1
    // is emitted in frame t = n - u.
    if (tid < 64)
        align_walk_bit_windows(bits, Up, tid, __builtin_amdgcn_readfirstlane(Ub), __builtin_amdgcn_readfirstlane(last),
                               [&](const int u, const int n) { fr[u - 1] = n - u; });
    __syncthreads();
    for (int uu = tid; uu < p.U - 1; uu += kThreads) {
        int f = -1;
        float lp = 0.0f;
        if (!bad && uu < Ub) {
            f = fr[uu];
            lp = cells[(size_t)((f + uu) % T) * Up + uu].y;
        }
        p.token_frames[(size_t)b * (p.U - 1) + uu] = f;
        p.token_logp[(size_t)b * (p.U - 1) + uu] = lp;
    }
}

hipError_t launch_align_path(const AlignParams &p, hipStream_t s) {
    return dispatch_align_path<2>(p.U, [&](auto K, auto G, auto WIDE) {
        constexpr bool kWide = decltype(WIDE)::value;
        hipLaunchKernelGGL((align_path_kernel<decltype(K)::value, decltype(G)::value, kWide>), dim3(p.B), dim3(kWide ? 1024 : 64), 0, s, p);
        return hipGetLastError();
    });
}

}  // namespace rnnt
