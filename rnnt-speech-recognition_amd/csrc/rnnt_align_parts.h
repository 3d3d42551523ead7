// rnnt_align_parts.h -- what the three forced-alignment kernel files share (align_kernels.hip, rnnt_modalign_kernels.hip,
// rnnt_tdtalign_kernels.hip; DESIGN.md sections 8i, 8n, 8v): the cell pass's (max, sum) arithmetic, chunk load, cell decomposition
// and lanes-per-cell dispatch, and the bit-lattice sweeps' lane shift, row loader, launch table and back-trace.  Plain inline
// functions: every kernel stays in its own file and its own library, with the launch shape, the resources and the order of every
// floating-point operation it had with its own copy (profiles/align_parts_notes.md).
//
// The bits of an alignment depend on the chunk-to-lane map, the merge order and the strict-greater tie rule.  The first two live
// here and nowhere else; the tie rule is in each sweep's own step.
#pragma once
#include "rnnt_align.h"

#include <math.h>
#include <type_traits>

namespace rnnt {

// ---------------------------------------------------------------------------------------------
// Cell pass.  A group of L lanes owns one lattice cell; lane j takes the 16-byte chunks j, j + L, j + 2L ... of the cell's logits
// and keeps a running (max, sum of exp(x - max)); the L partial pairs are merged by a butterfly.  The chunk-to-lane map and the
// merge order depend on the row length only, and the scalar-load variant (a length that is no multiple of 4, or an unaligned
// slab) pads its last chunk with -inf and follows the same map, so both give the same bits.
// ---------------------------------------------------------------------------------------------
constexpr float kAlignNegInit = -3.0e38f;  // finite: two lanes without elements merge to (this, 0), not to NaN

// chunk ch of a row of n floats
template <bool VEC>
__device__ __forceinline__ float4 align_load_chunk(const float *row, const int ch, const int n) {
    const int i = 4 * ch;
    if (VEC) return *reinterpret_cast<const float4 *>(row + i);
    float4 x;
    x.x = row[i];
    x.y = i + 1 < n ? row[i + 1] : -INFINITY;
    x.z = i + 2 < n ? row[i + 2] : -INFINITY;
    x.w = i + 3 < n ? row[i + 3] : -INFINITY;
    return x;
}

// the merge of two (max, sum) pairs across lanes `off` apart; the lower lane's part first on both sides: the same bits in both
__device__ __forceinline__ void align_merge(float &m, float &s, const int j, const int off) {
    const float m2 = __shfl_xor(m, off, 64), s2 = __shfl_xor(s, off, 64);
    const float nm = fmaxf(m, m2);
    const float a = s * __expf(m - nm), bsum = s2 * __expf(m2 - nm);
    s = (j & off) ? bsum + a : a + bsum;
    m = nm;
}

// (m, s) with m + log(s) the log-sum-exp of row[0 .. V), in every lane of the cell's group
template <int L, bool VEC>
__device__ __forceinline__ void align_cell_max_sum(const float *row, const int V, const int j, float &m, float &s) {
    const int chunks = (V + 3) >> 2;
    m = kAlignNegInit, s = 0.0f;
#pragma unroll 2
    for (int ch = j; ch < chunks; ch += L) {
        const float4 x = align_load_chunk<VEC>(row, ch, V);
        const float nm = fmaxf(m, fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w)));
        s = s * __expf(m - nm) + ((__expf(x.x - nm) + __expf(x.y - nm)) + (__expf(x.z - nm) + __expf(x.w - nm)));
        m = nm;
    }
#pragma unroll
    for (int off = L / 2; off >= 1; off >>= 1) align_merge(m, s, j, off);
}

// The cell of this thread's group in a launch of 256 / L cells per block over the slab [B][S][U]: c its index in the slab, (b, t, u)
// its place in the lattice, Tb, Ub the utterance's clamped lengths.  False outside the slab or the utterance's lattice: such a
// cell is not read (the whole group leaves together).
struct AlignCell {
    uint32_t c;
    int b, t, u, Tb, Ub;
};

template <int L, typename Params>
__device__ __forceinline__ bool align_cell_of(const Params &p, AlignCell &q) {
    const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.S * (uint32_t)p.U;
    q.c = blockIdx.x * (uint32_t)(256 / L) + (uint32_t)(threadIdx.x / L);
    if (q.c >= ncells) return false;
    const uint32_t bs = fdiv(q.c, p.divU);
    q.u = (int)(q.c - bs * (uint32_t)p.U);
    q.b = (int)fdiv(bs, p.divS);
    q.t = p.t0 + (int)(bs - (uint32_t)q.b * (uint32_t)p.S);
    q.Tb = min(max(p.input_lengths[q.b], 1), p.T);
    q.Ub = min(max(p.label_lengths[q.b], 0), p.U - 1);
    return q.t < q.Tb && q.u <= q.Ub;
}

// label u of utterance b, clamped into the vocabulary
template <typename Params>
__device__ __forceinline__ int align_label(const Params &p, const int b, const int u, const int V) {
    return min(max(p.labels[(size_t)b * (size_t)(p.U - 1) + u], 0), V - 1);
}

// blocks of the cell pass at L lanes per cell
template <typename Params>
inline uint32_t align_cells_grid(const Params &p, const uint32_t L) {
    const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.S * (uint32_t)p.U, per = 256 / L;
    return (ncells + per - 1) / per;
}

// Calls f(L) with the lanes per cell (as std::integral_constant): the smallest power of two that gives every 16-byte chunk of a cell
// a lane, at most one wavefront.
template <typename F>
inline hipError_t dispatch_cell_lanes(const int chunks, F &&f) {
    using std::integral_constant;
    if (chunks <= 1) return f(integral_constant<int, 1>());
    if (chunks <= 2) return f(integral_constant<int, 2>());
    if (chunks <= 4) return f(integral_constant<int, 4>());
    if (chunks <= 8) return f(integral_constant<int, 8>());
    if (chunks <= 16) return f(integral_constant<int, 16>());
    if (chunks <= 32) return f(integral_constant<int, 32>());
    return f(integral_constant<int, 64>());
}

// ---------------------------------------------------------------------------------------------
// The sweeps with one decision bit per node (standard and modified lattice): thread j owns the lattice columns j K ... j K + K - 1
// of rows of {lpb, lpl}, Up per row.
// ---------------------------------------------------------------------------------------------
// x of the lane below; `fill` in lane 0 (a whole-wave DPP shift)
__device__ __forceinline__ double align_from_lower_lane(const double x, const double fill) {
    const long long xi = __double_as_longlong(x), fi = __double_as_longlong(fill);
    const int lo = __builtin_amdgcn_update_dpp((int)fi, (int)xi, 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(fi >> 32), (int)(xi >> 32), 0x138, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

template <int K>
struct AlignRow {
    float2 e[K];
};

template <int K>
__device__ __forceinline__ void align_load_row(AlignRow<K> &d, const float2 *rowp) {
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

// Calls f(K, G, WIDE) (as std::integral_constant) for U lattice columns: K columns per thread, G rows in flight per buffer --
// about 32 cells of registers per thread and buffer --, one wavefront up to 1024 columns and 1024 threads with 128 registers each
// beyond.  WideG4: the G of the wide kernel at K = 4, the one entry in which the two lattices differ.
template <int WideG4, typename F>
inline hipError_t dispatch_align_path(const int U, F &&f) {
    using std::false_type;
    using std::integral_constant;
    using std::true_type;
    switch (sweep_K(U)) {
        case 1: return f(integral_constant<int, 1>(), integral_constant<int, 16>(), false_type());
        case 2: return f(integral_constant<int, 2>(), integral_constant<int, 16>(), false_type());
        case 3: return f(integral_constant<int, 3>(), integral_constant<int, 8>(), false_type());
        case 4: return f(integral_constant<int, 4>(), integral_constant<int, 8>(), false_type());
        case 6: return f(integral_constant<int, 6>(), integral_constant<int, 4>(), false_type());
        case 8: return f(integral_constant<int, 8>(), integral_constant<int, 4>(), false_type());
        case 12: return f(integral_constant<int, 12>(), integral_constant<int, 2>(), false_type());
        case 16: return f(integral_constant<int, 16>(), integral_constant<int, 2>(), false_type());
        default: break;
    }
    switch (align_wide_K(U)) {
        case 2: return f(integral_constant<int, 2>(), integral_constant<int, 2>(), true_type());
        case 3: return f(integral_constant<int, 3>(), integral_constant<int, 2>(), true_type());
        case 4: return f(integral_constant<int, 4>(), integral_constant<int, WideG4>(), true_type());
        case 6: return f(integral_constant<int, 6>(), integral_constant<int, 1>(), true_type());
        case 8: return f(integral_constant<int, 8>(), integral_constant<int, 1>(), true_type());
        default: return hipErrorInvalidValue;
    }
}

// Back-trace from node (column u, step n) down to step 1, on one wavefront with wave-uniform (scalar) state; bit (n mod 32) of
// bits[n / 32][u] says that the node was reached by its label arrival, and emit(u, n) is then called in lane 0.  Lane l holds the
// decision word of column wu - l of the current block of 32 steps; 32 steps move at most 32 columns, so a window of 64 columns
// anchored at the column the PREVIOUS block started from covers the block -- which is what lets the next block's window be loaded
// while this one is walked.  A step is a v_readlane and a few scalar instructions; no memory access is on the chain.
template <typename Emit>
__device__ __forceinline__ void align_walk_bit_windows(const uint32_t *bits, const int Up, const int lane, int u, int n, Emit &&emit) {
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
            if (bit && lane == 0) emit(u, n);
            u -= bit;
        }
        wcur = wnxt;
        wu_cur = wu_nxt;
    }
}

}  // namespace rnnt
