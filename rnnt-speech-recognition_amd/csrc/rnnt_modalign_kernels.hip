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
// Every sum has an order fixed by V alone in the cell pass and by the utterance's own cells in the sweep: an utterance's outputs
// do not depend on the batch around it nor on how the frames were cut into slabs.
#include "rnnt_modalign.h"

#include <math.h>

namespace rnnt {

// ---------------------------------------------------------------------------------------------
// Cell pass.  A group of L lanes owns one lattice cell; lane j takes the 16-byte chunks j, j + L, j + 2L ... of its V logits and
// keeps a running (max, sum of exp(x - max)); the L partial pairs are merged by a butterfly.  The chunk-to-lane map and the merge
// order depend on V only, and the scalar-load variant (V not a multiple of 4, or an unaligned slab) pads its last chunk with
// -inf and follows the same map, so both give the same bits.
// ---------------------------------------------------------------------------------------------
constexpr float kModAlignNegInit = -3.0e38f;  // finite: two lanes without elements merge to (this, 0), not to NaN

template <int L, bool VEC>
__global__ void __launch_bounds__(256) modalign_cells_kernel(const ModAlignParams p) {
    constexpr int kCellsPerBlock = 256 / L;
    const int tid = threadIdx.x;
    const int j = tid % L;
    const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.S * (uint32_t)p.U;
    const uint32_t c = blockIdx.x * (uint32_t)kCellsPerBlock + (uint32_t)(tid / L);
    if (c >= ncells) return;
    const uint32_t bs = fdiv(c, p.divU);
    const int u = (int)(c - bs * (uint32_t)p.U);
    const int b = (int)fdiv(bs, p.divS);
    const int t = p.t0 + (int)(bs - (uint32_t)b * (uint32_t)p.S);
    int Tb = p.input_lengths[b], Ub = p.label_lengths[b];
    Tb = min(max(Tb, 1), p.T);
    Ub = min(max(Ub, 0), p.U - 1);
    // outside the utterance's lattice, or no path passes here: not read (the whole group leaves together)
    if (t >= Tb || u > Ub || u > t || Ub - u > Tb - t) return;

    const int V = p.V;
    const float *row = p.acts + (size_t)c * (size_t)V;
    const int chunks = (V + 3) >> 2;
    float m = kModAlignNegInit, s = 0.0f;
#pragma unroll 2
    for (int ch = j; ch < chunks; ch += L) {
        float4 x;
        if (VEC) {
            x = *reinterpret_cast<const float4 *>(row + 4 * ch);
        } else {
            const int i = 4 * ch;
            x.x = row[i];
            x.y = i + 1 < V ? row[i + 1] : -INFINITY;
            x.z = i + 2 < V ? row[i + 2] : -INFINITY;
            x.w = i + 3 < V ? row[i + 3] : -INFINITY;
        }
        const float nm = fmaxf(m, fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w)));
        s = s * __expf(m - nm) + ((__expf(x.x - nm) + __expf(x.y - nm)) + (__expf(x.z - nm) + __expf(x.w - nm)));
        m = nm;
    }
#pragma unroll
    for (int off = L / 2; off >= 1; off >>= 1) {
        const float m2 = __shfl_xor(m, off, 64), s2 = __shfl_xor(s, off, 64);
        const float nm = fmaxf(m, m2);
        const float a = s * __expf(m - nm), bsum = s2 * __expf(m2 - nm);
        s = (j & off) ? bsum + a : a + bsum;  // lower lane's part first on both sides: the pair ends with the same bits
        m = nm;
    }
    if (j != 0) return;
    const float lse = m + __logf(s);
    float2 out;
    out.x = row[p.blank] - lse;
    out.y = 0.0f;
    if (u < Ub) {
        int lab = p.labels[(size_t)b * (size_t)(p.U - 1) + u];
        lab = min(max(lab, 0), V - 1);
        out.y = row[lab] - lse;
    }
    p.lp[((size_t)b * p.T + t) * (size_t)p.Up + u] = out;
}

template <int L>
static hipError_t launch_cells_L(const ModAlignParams &p, bool vec, hipStream_t s) {
    const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.S * (uint32_t)p.U;
    const uint32_t per = 256 / L;
    const uint32_t grid = (ncells + per - 1) / per;
    if (vec)
        hipLaunchKernelGGL((modalign_cells_kernel<L, true>), dim3(grid), dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((modalign_cells_kernel<L, false>), dim3(grid), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_modalign_cells(const ModAlignParams &p, hipStream_t s) {
    const int chunks = (p.V + 3) / 4;
    const bool vec = (p.V % 4 == 0) && (((uintptr_t)p.acts & 15) == 0);
    // lanes per cell: the smallest power of two that gives every 16-byte chunk of a cell a lane, at most one wavefront
    if (chunks <= 1) return launch_cells_L<1>(p, vec, s);
    if (chunks <= 2) return launch_cells_L<2>(p, vec, s);
    if (chunks <= 4) return launch_cells_L<4>(p, vec, s);
    if (chunks <= 8) return launch_cells_L<8>(p, vec, s);
    if (chunks <= 16) return launch_cells_L<16>(p, vec, s);
    if (chunks <= 32) return launch_cells_L<32>(p, vec, s);
    return launch_cells_L<64>(p, vec, s);
}

// ---------------------------------------------------------------------------------------------
// Sweep + back-trace.  Thread j owns the lattice columns j K ... j K + K - 1.  Step t takes row t of {lpb, lpl} and the values of
// the nodes of row t to those of row t + 1: node (t, u) offers v + lpb to (t + 1, u) -- the same column -- and v + lpl to
// (t + 1, u + 1) -- the next column; only the last column's label offer crosses to the next thread (a whole-wave DPP shift, or
// LDS + one barrier per row in the wide kernel).  The tie rule of include/rnnt_modified_align.h: the label arrival wins only if
// STRICTLY greater.  Nodes outside the band are -inf, and the {lpb, lpl} of cells outside it (never written by the cell pass)
// are selected away before any arithmetic.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double modalign_from_lower_lane(const double x, const double fill) {
    const long long xi = __double_as_longlong(x), fi = __double_as_longlong(fill);
    const int lo = __builtin_amdgcn_update_dpp((int)fi, (int)xi, 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(fi >> 32), (int)(xi >> 32), 0x138, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

template <int K>
struct ModAlignRow {
    float2 e[K];
};

template <int K>
__device__ __forceinline__ void modalign_load_row(ModAlignRow<K> &d, const float2 *rowp) {
    if constexpr (K % 2 == 0) {
        const float4 *q = reinterpret_cast<const float4 *>(rowp);  // 8 K bytes per thread, 16-byte aligned (K even)
#pragma unroll
        for (int k = 0; k < K / 2; ++k) {
            const float4 x = q[k];
            d.e[2 * k] = make_float2(x.x, x.y);
            d.e[2 * k + 1] = make_float2(x.z, x.w);
        }
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) d.e[k] = rowp[k];
    }
}

template <int K, int G, bool WIDE>
__global__ void __launch_bounds__(WIDE ? 1024 : 64) modalign_path_kernel(const ModAlignParams p) {
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
    const float2 *lp = p.lp + (size_t)b * p.T * (size_t)Up;
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
    auto load_block = [&](ModAlignRow<K>(&buf)[G]) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int s = min(ls, Tb - 1);  // (past the end: a row of this utterance again, not used)
            modalign_load_row<K>(buf[g], lp + (size_t)s * Up + u0);
            ++ls;
        }
    };
    // one row: d = the cells of row t, the edges into the nodes of row t + 1
    auto step = [&](const int t, const ModAlignRow<K> &d) {
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
            cin = modalign_from_lower_lane(move[K - 1], -INFINITY);
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

    ModAlignRow<K> bufA[G], bufB[G];
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

    // Back-trace: T_b dependent steps, on wave 0 with wave-uniform (scalar) state.  Lane l holds the decision word of column
    // wu - l of the current block of 32 rows; 32 steps move at most 32 columns, so a window of 64 columns anchored at the column
    // the PREVIOUS block started from covers the block -- which is what lets the next block's window be loaded while this one is
    // walked.  A step is a v_readlane and a few scalar instructions; no memory access is on the chain.
    if (tid < 64) {
        const int lane = tid;
        int u = __builtin_amdgcn_readfirstlane(Ub), t = __builtin_amdgcn_readfirstlane(Tb);
        auto load_window = [&](const int blk, const int wu) -> uint32_t {
            const int col = wu - lane;
            return (blk >= 0 && col >= 0) ? bits[(size_t)blk * Up + col] : 0u;
        };
        int blk = t >> 5, wu_cur = u;
        uint32_t wcur = load_window(blk, wu_cur);
        for (; blk >= 0; --blk) {
            const int wu_nxt = u;
            const uint32_t wnxt = load_window(blk - 1, wu_nxt);
            const int tlo = max(blk * 32, 1);
            for (; t >= tlo; --t) {
                const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)wcur, __builtin_amdgcn_readfirstlane(wu_cur - u));
                const int bit = (int)((word >> (t & 31)) & 1u);
                if (bit && lane == 0) fr[u - 1] = t - 1;  // the label arrival into (t, u): token u - 1 is emitted in frame t - 1
                u -= bit;
            }
            wcur = wnxt;
            wu_cur = wu_nxt;
        }
    }
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

template <int K, int G, bool WIDE>
static hipError_t launch_path_KG(const ModAlignParams &p, hipStream_t s) {
    hipLaunchKernelGGL((modalign_path_kernel<K, G, WIDE>), dim3(p.B), dim3(WIDE ? 1024 : 64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_modalign_path(const ModAlignParams &p, hipStream_t s) {
    // rows in flight per buffer: about 32 cells of registers per thread and buffer
    switch (sweep_K(p.U)) {
        case 1: return launch_path_KG<1, 16, false>(p, s);
        case 2: return launch_path_KG<2, 16, false>(p, s);
        case 3: return launch_path_KG<3, 8, false>(p, s);
        case 4: return launch_path_KG<4, 8, false>(p, s);
        case 6: return launch_path_KG<6, 4, false>(p, s);
        case 8: return launch_path_KG<8, 4, false>(p, s);
        case 12: return launch_path_KG<12, 2, false>(p, s);
        case 16: return launch_path_KG<16, 2, false>(p, s);
        default: break;
    }
    switch (align_wide_K(p.U)) {  // more than 1024 columns: 1024 threads, 128 registers each
        case 2: return launch_path_KG<2, 2, true>(p, s);
        case 3: return launch_path_KG<3, 2, true>(p, s);
        case 4: return launch_path_KG<4, 1, true>(p, s);
        case 6: return launch_path_KG<6, 1, true>(p, s);
        case 8: return launch_path_KG<8, 1, true>(p, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace rnnt
