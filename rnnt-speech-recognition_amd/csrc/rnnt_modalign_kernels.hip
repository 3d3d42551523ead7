// rnnt_modalign_kernels.hip -- forced alignment on the MODIFIED lattice: the maximum-probability path among those that emit
// exactly one of {blank, next label} per frame (include/rnnt_modified_align.h; rnnt_modalign.h for the workspace; DESIGN.md
// section 8n).
//
//   modalign_cells_kernel<L, VEC>   one pass over a slab of logits: log-softmax normaliser per in-band cell (f32, online max /
//                                   sum, L lanes per cell), written as {lpb, lpl} row-major [t][u].  HBM-bound.
//   modalign_path_kernel<K, G, W>   one workgroup per utterance: max-plus sweep over the rows in float64 registers (K lattice
//                                   columns per thread; one wavefront up to 1024 columns, 1024 threads beyond), one decision bit
//                                   per node, then the back-trace (wave 0, scalar walk over register-held bit windows) and the
//                                   three outputs.
//
// The normaliser, the cell decomposition, the lane dispatch, the DPP shift, the row loader, the <K, G, W> table and the back-trace
// are those of rnnt_align_parts.h, shared with the standard and the TDT aligner, and the kernel argument is the standard aligner's
// AlignParams; what is here is this lattice's own: the band, the row-order step with its masks, the score and the outputs.
//
// Every sum has an order fixed by V alone in the cell pass and by the utterance's own cells in the sweep: an utterance's outputs
// do not depend on the batch around it nor on how the frames were cut into slabs.
#include "rnnt_align_parts.h"
#include "rnnt_modalign.h"

namespace rnnt {

// Cell pass (rnnt_align_parts.h): {lpb, lpl} of every cell inside the band.
template <int L, bool VEC>
__global__ void __launch_bounds__(256) modalign_cells_kernel(const AlignParams p) {
    const int j = threadIdx.x % L;
    AlignCell q;
    // outside the utterance's lattice, or no path passes here: not read (the whole group leaves together)
    if (!align_cell_of<L>(p, q) || q.u > q.t || q.Ub - q.u > q.Tb - q.t) return;
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
    p.cells[((size_t)b * p.T + t) * (size_t)p.Up + u] = out;
}

hipError_t launch_modalign_cells(const AlignParams &p, hipStream_t s) {
    const bool vec = (p.V % 4 == 0) && (((uintptr_t)p.acts & 15) == 0);
    return dispatch_cell_lanes((p.V + 3) / 4, [&](auto L) {
        constexpr int kL = decltype(L)::value;
        if (vec)
            hipLaunchKernelGGL((modalign_cells_kernel<kL, true>), dim3(align_cells_grid(p, kL)), dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((modalign_cells_kernel<kL, false>), dim3(align_cells_grid(p, kL)), dim3(256), 0, s, p);
        return hipGetLastError();
    });
}

// ---------------------------------------------------------------------------------------------
// Sweep + back-trace.  Thread j owns the lattice columns j K ... j K + K - 1.  Step t takes row t of {lpb, lpl} and the values of
// the nodes of row t to those of row t + 1: node (t, u) offers v + lpb to (t + 1, u) -- the same column -- and v + lpl to
// (t + 1, u + 1) -- the next column; only the last column's label offer crosses to the next thread (a whole-wave DPP shift, or
// LDS + one barrier per row in the wide kernel).  The tie rule of include/rnnt_modified_align.h: the label arrival wins only if
// STRICTLY greater.  Nodes outside the band are -inf, and the {lpb, lpl} of cells outside it (never written by the cell pass)
// are selected away before any arithmetic.
// ---------------------------------------------------------------------------------------------
template <int K, int G, bool WIDE>
__global__ void __launch_bounds__(WIDE ? 1024 : 64) modalign_path_kernel(const AlignParams p) {
    constexpr int kThreads = WIDE ? 1024 : 64;
    constexpr int kFrames = WIDE ? kMaxU : 1024;
    __shared__ int fr[kFrames];                  // emission frame per token, written by the back-trace
    __shared__ double xch[WIDE ? 2 * 1024 : 2];  // the wide kernel's neighbour exchange, double-buffered by row parity
    const int b = blockIdx.x, tid = threadIdx.x;
    int Tb = p.input_lengths[b], Ub = p.label_lengths[b];
    const bool bad = Tb < 1 || Tb > p.T || Ub < 0 || Ub > p.U - 1;
    Tb = min(max(Tb, 1), p.T);
    Ub = min(max(Ub, 0), p.U - 1);
    int *out_frames = p.token_frames + (size_t)b * (p.U - 1);
    float *out_logp = p.token_logp + (size_t)b * (p.U - 1);

    if (bad || Ub > Tb) {  // out-of-range lengths: NaN; more labels than frames: no path, -inf.  The workspace is not read.
        for (int uu = tid; uu < p.U - 1; uu += kThreads) {
            out_frames[uu] = -1;
            out_logp[uu] = 0.0f;
        }
        if (tid == 0) p.scores[b] = bad ? __int_as_float(0x7fc00000) : -INFINITY;
        return;
    }

    const int Up = p.Up;
    const int u0 = tid * K;
    const float2 *lp = p.cells + (size_t)b * p.T * (size_t)Up;
    uint32_t *bits = p.bits + (size_t)b * p.NB * (size_t)Up;
    auto in_band = [&](const int t, const int u) { return u <= t && u <= Ub && Ub - u <= Tb - t; };

    double v[K];    // row 0
    uint32_t w[K];  // the decision bits of the current block of 32 rows
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = (u0 + k == 0) ? 0.0 : -INFINITY;
        w[k] = 0u;
    }
    for (int uu = tid; uu < kFrames; uu += kThreads) fr[uu] = 0;  // (a NaN lattice may leave tokens unvisited: keep reads in bounds)

    int ls = 0;  // the next row to load
    auto load_block = [&](AlignRow<K>(&buf)[G]) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int s = min(ls, Tb - 1);  // (past the end: a row of this utterance again, not used)
            align_load_row<K>(buf[g], lp + (size_t)s * Up + u0);
            ++ls;
        }
    };
    // one row: d = the cells of row t, the edges into the nodes of row t + 1
    auto step = [&](const int t, const AlignRow<K> &d) {
        double stay[K], move[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int u = u0 + k;
            const bool ok = in_band(t, u);
            stay[k] = ok ? v[k] + (double)d.e[k].x : -INFINITY;
            move[k] = (ok && u < Ub) ? v[k] + (double)d.e[k].y : -INFINITY;
        }
        double cin;
        if constexpr (WIDE) {
            double *x = xch + (t & 1) * 1024;
            x[tid] = move[K - 1];
            __syncthreads();
            cin = tid ? x[tid - 1] : -INFINITY;
        } else {
            cin = align_from_lower_lane(move[K - 1], -INFINITY);
        }
        const int r = t + 1;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double from = k ? move[k - 1] : cin;
            const bool dst_ok = in_band(r, u0 + k);
            const bool lab = from > stay[k];  // strictly greater: an exact tie takes the blank arrival
            v[k] = dst_ok ? (lab ? from : stay[k]) : -INFINITY;
            w[k] |= (uint32_t)(lab && dst_ok) << (r & 31);
        }
        if ((r & 31) == 31 || r == Tb) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                bits[(size_t)(r >> 5) * Up + u0 + k] = w[k];
                w[k] = 0u;
            }
        }
    };

    AlignRow<K> bufA[G], bufB[G];
    load_block(bufA);
    for (int s0 = 0; s0 < Tb; s0 += 2 * G) {
        load_block(bufB);
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (s0 + g < Tb) step(s0 + g, bufA[g]);
        load_block(bufA);
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (s0 + G + g < Tb) step(s0 + G + g, bufB[g]);
    }

    // the score: v(T_b, L_b), no final blank
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (u0 + k == Ub) p.scores[b] = (float)v[k];
    __threadfence();  // the decision words are read back by other lanes below
    __syncthreads();

    // Back-trace (rnnt_align_parts.h): T_b dependent steps on wave 0.  A set bit of row t in column u is the label arrival into
    // (t, u): token u - 1 is emitted in frame t - 1.
    if (tid < 64)
        align_walk_bit_windows(bits, Up, tid, __builtin_amdgcn_readfirstlane(Ub), __builtin_amdgcn_readfirstlane(Tb),
                               [&](const int u, const int t) { fr[u - 1] = t - 1; });
    __syncthreads();
    for (int uu = tid; uu < p.U - 1; uu += kThreads) {
        int f = -1;
        float l = 0.0f;
        if (uu < Ub) {
            f = fr[uu];
            l = lp[(size_t)f * Up + uu].y;
        }
        out_frames[uu] = f;
        out_logp[uu] = l;
    }
}

hipError_t launch_modalign_path(const AlignParams &p, hipStream_t s) {
    return dispatch_align_path<1>(p.U, [&](auto K, auto G, auto WIDE) {
        constexpr bool kWide = decltype(WIDE)::value;
        hipLaunchKernelGGL((modalign_path_kernel<decltype(K)::value, decltype(G)::value, kWide>), dim3(p.B), dim3(kWide ? 1024 : 64), 0, s, p);
        return hipGetLastError();
    });
}

}  // namespace rnnt
