// align_kernels.hip -- forced alignment: the maximum-probability monotone path through the T x (U+1) lattice the loss sums over
// (include/rnnt.h "Forced alignment").
//
//   align_cells_kernel<L, VEC>   one pass over a slab of logits: log-softmax normaliser per lattice cell (f32, online max / sum,
//                                L lanes per cell), written as {lpb, lpl} on the wrapped-skew grid of rnnt_align.h.  HBM-bound.
//   align_path_kernel<K, G, W>   one workgroup per utterance: max-plus sweep over the anti-diagonals in float64 registers (K lattice
//                                columns per thread; one wavefront up to 1024 columns, 1024 threads beyond), one decision bit per
//                                cell, then the back-trace (wave 0, scalar walk over register-held bit windows) and the outputs.
//
// Every sum has an order fixed by (V) alone in the cell pass and by the utterance's own cells in the sweep: an utterance's outputs
// do not depend on the batch around it nor on how the frames were cut into slabs.
#include "rnnt_align.h"

#include <math.h>

namespace rnnt {

// ---------------------------------------------------------------------------------------------
// Cell pass.  A group of L lanes owns one lattice cell; lane j takes the 16-byte chunks j, j + L, j + 2L ... of its V logits and
// keeps a running (max, sum of exp(x - max)); the L partial pairs are merged by a butterfly.  The chunk-to-lane map and the merge
// order depend on V only, and the scalar-load variant (V not a multiple of 4, or an unaligned tensor) follows the same map, so
// both give the same bits.
// ---------------------------------------------------------------------------------------------
constexpr float kAlignNegInit = -3.0e38f;  // finite: two lanes without elements merge to (this, 0), not to NaN

template <int L, bool VEC>
__global__ void __launch_bounds__(256) align_cells_kernel(const AlignParams p) {
    constexpr int kCellsPerBlock = 256 / L;
    const int tid = threadIdx.x;
    const int j = tid % L;
    const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.S * (uint32_t)p.U;
    const uint32_t c = blockIdx.x * (uint32_t)kCellsPerBlock + (uint32_t)(tid / L);
    if (c >= ncells) return;
    const uint32_t bt = fdiv(c, p.divU);
    const int u = (int)(c - bt * (uint32_t)p.U);
    const int b = (int)fdiv(bt, p.divS);
    const int t = p.t0 + (int)(bt - (uint32_t)b * (uint32_t)p.S);
    int Tb = p.input_lengths[b], Ub = p.label_lengths[b];
    Tb = min(max(Tb, 1), p.T);
    Ub = min(max(Ub, 0), p.U - 1);
    if (t >= Tb || u > Ub) return;  // outside the utterance's lattice: not read (the whole group leaves together)

    const int V = p.V;
    const float *row = p.acts + (size_t)c * (size_t)V;
    const int chunks = (V + 3) >> 2;
    float m = kAlignNegInit, s = 0.0f;
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
    int r = t + u;  // wrapped skew: diagonal n = t + u lives in row n mod T
    r = r >= p.T ? r % p.T : r;
    p.cells[((size_t)b * p.T + r) * (size_t)p.Up + u] = out;
}

template <int L>
static hipError_t launch_cells_L(const AlignParams &p, bool vec, hipStream_t s) {
    const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.S * (uint32_t)p.U;
    const uint32_t per = 256 / L;
    const uint32_t grid = (ncells + per - 1) / per;
    if (vec)
        hipLaunchKernelGGL((align_cells_kernel<L, true>), dim3(grid), dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((align_cells_kernel<L, false>), dim3(grid), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_align_cells(const AlignParams &p, hipStream_t s) {
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
// Sweep + back-trace.  Thread j owns the lattice columns j K ... j K + K - 1.  "Push" form of the recurrence: a cell of diagonal
// n - 1 with value v offers v + lpb to (t + 1, u) -- the same column -- and v + lpl to (t, u + 1) -- the next column --, both on
// diagonal n; only the last column's label offer crosses to the next thread (a whole-wave DPP shift, or LDS + one barrier per
// diagonal in the wide kernel).  The tie rule of include/rnnt.h: the label arrival wins only if STRICTLY greater.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double align_from_lower_lane(const double x, const double fill) {
    const long long xi = __double_as_longlong(x), fi = __double_as_longlong(fill);
    const int lo = __builtin_amdgcn_update_dpp((int)fi, (int)xi, 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(fi >> 32), (int)(xi >> 32), 0x138, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

template <int K>
struct AlignDiag {
    float2 e[K];
};

template <int K>
__device__ __forceinline__ void align_load_diag(AlignDiag<K> &d, const float2 *rowp) {
    if constexpr (K % 2 == 0) {
        const float4 *q = reinterpret_cast<const float4 *>(rowp);  // 16 K bytes per thread, 16-byte aligned (K even)
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
    auto load_block = [&](AlignDiag<K>(&buf)[G]) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            align_load_diag<K>(buf[g], cells + (size_t)lrow * Up + u0);
            lrow = (lrow + 1 == T) ? 0 : lrow + 1;
        }
    };
    // one diagonal: n = destination diagonal, d = the cells of diagonal n - 1
    auto step = [&](const int n, const AlignDiag<K> &d) {
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

    AlignDiag<K> bufA[G], bufB[G];
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

    // Back-trace: T_b + U_b - 1 dependent steps, on wave 0 with wave-uniform (scalar) state.  Lane l holds the decision word of
    // column wu - l of the current block of 32 diagonals; 32 steps move at most 32 columns, so a window of 64 columns anchored at
    // the column the PREVIOUS block started from covers the block -- which is what lets the next block's window be loaded while
    // this one is walked.  A step is a v_readlane and a few scalar instructions; no memory access is on the chain.
    if (tid < 64) {
        const int lane = tid;
        int u = __builtin_amdgcn_readfirstlane(Ub), n = __builtin_amdgcn_readfirstlane(last);
        auto load_window = [&](const int blk, const int wu) -> uint32_t {
            const int col = wu - lane;
            return (blk >= 0 && col >= 0) ? bits[(size_t)blk * Up + col] : 0u;
        };
        int blk = n >> 5, wu_cur = u;
        uint32_t wcur = load_window(blk, wu_cur);
        for (; blk >= 0; --blk) {
            const int wu_nxt = u;
            const uint32_t wnxt = load_window(blk - 1, wu_nxt);
            const int nlo = max(blk * 32, 1);
            for (; n >= nlo; --n) {
                const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)wcur, __builtin_amdgcn_readfirstlane(wu_cur - u));
                const int bit = (int)((word >> (n & 31)) & 1u);
                if (bit && lane == 0) fr[u - 1] = n - u;  // token u - 1 is emitted in frame t = n - u
                u -= bit;
            }
            wcur = wnxt;
            wu_cur = wu_nxt;
        }
    }
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

template <int K, int G, bool WIDE>
static hipError_t launch_path_KG(const AlignParams &p, hipStream_t s) {
    hipLaunchKernelGGL((align_path_kernel<K, G, WIDE>), dim3(p.B), dim3(WIDE ? 1024 : 64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_align_path(const AlignParams &p, hipStream_t s) {
    // diagonals in flight per buffer: about 32 cells of registers per thread and buffer
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
        case 4: return launch_path_KG<4, 2, true>(p, s);
        case 6: return launch_path_KG<6, 1, true>(p, s);
        case 8: return launch_path_KG<8, 1, true>(p, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace rnnt
