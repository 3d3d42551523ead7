// rnnt_tdt_joint_kernels.hip -- the fused TDT joint: costs and the four gradients of the token-and-duration transducer loss from
// the projections, without the logits [B, T, U, V + D] or any per-cell [J] array ever existing in memory
// (include/rnnt_tdt_joint.h; rnnt_tdt_joint.h for the workspace).  The lattice sweeps are
// rnnt_tdt_kernels.hip's, unchanged; the split-precision joint is rnnt_pruned_joint_kernels.hip's arithmetic on another tiling.
//
//   tj_w2max_kernel      abs-max of W2 in 64 per-block entries: the power of two s2 that puts max |s2 W2| into [2^13, 2^14)
//   tj_fwd_kernel        a workgroup = one frame t by 32 consecutive lattice columns of one utterance.  h = tanh(enc[t] + pred[u])
//                        is formed in the loader, behind the liveness test, and kept in LDS as binary16 hi + lo.  The logits exist
//                        32 columns at a time: the four waves split the J sum of a 32 x 32 tile (hi.hi + lo.hi + hi.lo on
//                        v_mfma_f32_32x32x16_f16, f32 accumulation), the partial tiles meet in LDS and eight lanes per row carry
//                        TWO online log-softmaxes across the tiles, one for the columns < V and one for the columns >= V (a tile
//                        that holds column V feeds both, by a column mask).  Stores the 2 D edge weights into the skewed planes
//                        of rnnt_tdt.h and both denominators as hi + lo.
//   tj_occ_kernel        per live cell {g_b, g_l, g_0 ... g_{D-1}} of rnnt_tdt.h at unit cost_scale, from alpha, the weights, the
//                        targets' betas and lnP: the edge logic is here and nowhere else in the backward
//   tj_bwd_dh_kernel     workgroup = (utterance, column tile, chunk of 32 frames).  Per frame: h and the logits tile by tile
//                        again, dlogits from the occupancy record and the denominators (scaled by 2^12 and split),
//                        dh += dlogits . W2^T on the MFMAs (a wave owns J / 32 / 4 column tiles of dh), dz = cost_scale dh (1 - h^2)
//                        in registers: its sum over the tile's 32 rows goes to encpart[b][t][column tile], its running sum over
//                        the chunk's frames to predpart[b][chunk][u], written once.  dz is never stored.
//   tj_reduce_enc_kernel d_enc_proj[b, t] = the column tiles' partials in column order; zeros for t >= T_b
//   tj_reduce_pred_kernel d_pred_proj[b, u] = the chunks' partials in frame order; zeros for u > L_b
//   tj_bwd_dw_kernel     workgroup (logit column tile, row chunk): recomputes h and the tile's logits for every row tile of its
//                        chunk, dW2 partial += h^T . dlogits on the MFMAs (dlogits carry cost_scale and one power of two for the
//                        whole batch), db2 partial = column sums; one partial per chunk
//   tj_reduce_w_kernel   dW2 / db2 = the partials summed in chunk order
//
// A tile whose live cells all have EXACTLY zero mass (g_b + g_l == 0) contributes nothing and is skipped by both MFMA kernels of
// the backward; there is no threshold above zero.  No atomics, no memset; every sum has an order fixed by the shapes, and a tile
// holds one utterance's rows alone: costs, d_enc_proj and d_pred_proj of an utterance do not depend on the batch around it.
//
// THE LIVENESS TEST COMES FIRST.  No address into enc_proj, pred_proj, the labels or the per-cell arrays is formed for a row
// that is not live.
#include "rnnt_tdt_joint.h"

#include <math.h>

namespace rnnt {

typedef _Float16 tjf16;
typedef _Float16 tjh4 __attribute__((ext_vector_type(4)));
typedef _Float16 tjh8 __attribute__((ext_vector_type(8)));
typedef float tjf32x16 __attribute__((ext_vector_type(16)));

constexpr int kTJThreads = 256;           // four waves
constexpr int kTJPad = 8;                 // binary16 elements of padding per h row: rows stay 16-byte aligned
constexpr int kTJStage = 33;              // row stride of the f32 staging tiles
constexpr int kTJDlPad = 40;              // row stride (binary16) of the dlogits tiles: 80 bytes, 16-byte aligned
constexpr int kTJRowF = 16;               // floats per row of the per-row record in LDS
constexpr float kTJNegInit = -3.0e38f;    // finite: lanes without columns merge to (this, 0), not to NaN
constexpr float kTJDlScale = 4096.0f;     // unit-scale dlogits (|.| <= 2) times 2^12 before the binary16 split
constexpr int kTJW2Log2 = 14;             // max |s2 W2| < 2^14
constexpr int kTJMaxScaleLog2 = 100;      // no power-of-two scale beyond 2^100
// the per-row record: what dlogits needs of a row (backward), or the logits the edge weights need (forward)
enum { kLseV = 0, kLoV = 1, kLseD = 2, kLoD = 3, kCoef = 4, kGb = 5, kGl = 6, kXb = 0, kXl = 1, kPerDur = 8 };

// row of accumulator register `reg` in a 32 x 32 result (the column is lane & 31)
__device__ __forceinline__ constexpr int tj_cd_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

__device__ __forceinline__ void tj_split(const float x, tjf16 &hi, tjf16 &lo) {
    hi = (tjf16)x;
    lo = (tjf16)(x - (float)hi);
}

__device__ __forceinline__ tjf32x16 tj_mfma3(const tjh8 ahi, const tjh8 alo, const tjh8 bhi, const tjh8 blo, tjf32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, bhi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, bhi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, blo, acc, 0, 0, 0);
    return acc;
}

// tanh(x) = sign(x) (1 - 2 / (1 + e^{2|x|})): saturates at +-inf; the exponent 2|x| log2(e) is formed as hi + lo so that the
// absolute error stays below ~1e-7 on both sides (the derivation: rnnt_pruned_joint_kernels.hip pj_tanh)
__device__ __forceinline__ float tj_tanh(const float x) {
    const float a = 2.0f * fabsf(x);
    const float L = 1.44269502162933349609375f, Llo = 1.925963033500011e-8f;  // log2(e) = L + Llo
    const float th = a * L;
    const float tl = fmaf(a, L, -th) + a * Llo;
    float e = __builtin_amdgcn_exp2f(th);
    if (e < 3.0e38f) e = fmaf(e, tl * 0.693147182464599609375f, e);
    return copysignf(1.0f - 2.0f / (1.0f + e), x);
}

// ---------------------------------------------------------------------------------------------
// abs-max of W2 (bit pattern of the non-negative float: unsigned order = float order; NaN / inf count as huge)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTJThreads) tj_w2max_kernel(const TdtJointParams p) {
    __shared__ unsigned red[4];
    const size_t n = (size_t)p.J * (size_t)p.R;
    unsigned m = 0u;
    for (size_t i = (size_t)blockIdx.x * kTJThreads + threadIdx.x; i < n; i += (size_t)kTJAbsBlocks * kTJThreads)
        m = max(m, __float_as_uint(p.W2[i]) & 0x7fffffffu);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    // these few words are rewritten by every call and read by every workgroup of the next kernels: agent-scope accesses on
    // both sides, so that no launch path (a graph replay included) can serve a reader a previous call's entries
    if (threadIdx.x == 0)
        __hip_atomic_store(p.w2max + blockIdx.x, max(max(red[0], red[1]), max(red[2], red[3])), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// s2 = 2^(14 - e) with max |W2| < 2^e; 1 for an all-zero or non-finite W2 (the products then carry the inf / NaN through).
// Every wave of a consumer redoes this: one entry per lane.
__device__ __forceinline__ float tj_w2_scale(const TdtJointParams &p) {
    unsigned m = __hip_atomic_load(p.w2max + (threadIdx.x & 63), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
    const float x = __uint_as_float(m);
    if (!(x > 0.f) || !(x < 3.0e38f)) return 1.0f;
    return ldexpf(1.0f, min(kTJW2Log2 - (ilogbf(x) + 1), kTJMaxScaleLog2));
}

// ---------------------------------------------------------------------------------------------
// The rows of a tile.
// ---------------------------------------------------------------------------------------------
struct TJUtt {
    int b, Tb, Lb;  // clamped into the tensors
    bool bad;       // out-of-range lengths: the utterance is reported as NaN
};

__device__ __forceinline__ TJUtt tj_utt(const TdtParams &q, const int b) {
    TJUtt m;
    m.b = b;
    const int Tb = q.input_lengths[b], Lb = q.label_lengths[b];
    m.bad = Tb < 1 || Tb > q.T || Lb < 0 || Lb > q.U - 1;
    m.Tb = min(max(Tb, 1), q.T);
    m.Lb = min(max(Lb, 0), q.U - 1);
    return m;
}

// LDS carve (bytes), shared by the three tile kernels
struct TJSmem {
    tjf16 *hhi, *hlo;    // [32][J + 8]
    float *part;         // [4][32][33]: the waves' partial logits tiles
    float *stage;        // [32][33]
    tjf16 *dlhi, *dllo;  // [32][40]
    int *row_live, *row_lab;  // [32]
    float *rowf;         // [32][16]: the per-row record
};
__host__ __device__ inline size_t tj_smem_bytes(const int J) {
    return (size_t)2 * kTJRows * (J + kTJPad) * 2 + (size_t)4 * kTJRows * kTJStage * 4 + (size_t)kTJRows * kTJStage * 4 +
           (size_t)2 * kTJRows * kTJDlPad * 2 + (size_t)2 * kTJRows * 4 + (size_t)kTJRows * kTJRowF * 4;
}
__device__ __forceinline__ TJSmem tj_carve(char *sm, const int J) {
    TJSmem s;
    s.hhi = (tjf16 *)sm;
    s.hlo = s.hhi + kTJRows * (J + kTJPad);
    s.part = (float *)(s.hlo + kTJRows * (J + kTJPad));
    s.stage = s.part + 4 * kTJRows * kTJStage;
    s.dlhi = (tjf16 *)(s.stage + kTJRows * kTJStage);
    s.dllo = s.dlhi + kTJRows * kTJDlPad;
    s.row_live = (int *)(s.dllo + kTJRows * kTJDlPad);
    s.row_lab = s.row_live + kTJRows;
    s.rowf = (float *)(s.row_lab + kTJRows);
    return s;
}

// threads 0 ... 31: the rows of tile (t, ct) of utterance m.b (t < m.Tb is the caller's) and, for the gradient kernels, what
// dlogits needs of each; `scale` multiplies the occupancy record.  Every thread of the workgroup calls it: it ends in a barrier
// and returns whether some live row of the tile carries mass (g_b + g_l != 0; NaN counts).
template <bool GRAD>
__device__ __forceinline__ bool tj_rows(const TdtJointParams &p, const TJSmem &sm, const TJUtt &m, const int t, const int ct, const float scale) {
    const TdtParams &q = p.lat;
    const int r = threadIdx.x;
    int mass = 0;
    if (r < kTJRows) {
        const int u = ct * kTJRows + r;
        const bool live = u <= m.Lb;
        int lab = -1;
        if (live && u < m.Lb) {
            lab = q.labels[(size_t)m.b * (size_t)(q.U - 1) + (size_t)u];
            lab = min(max(lab, 0), q.V - 1);
        }
        sm.row_live[r] = live ? 1 : 0;
        sm.row_lab[r] = lab;
        if constexpr (GRAD) {
            float *f = sm.rowf + r * kTJRowF;
            float2 lse = make_float2(0.f, 0.f), lo = make_float2(0.f, 0.f);
            float gb = 0.f, gl = 0.f;
#pragma unroll
            for (int i = 0; i < kTdtMaxD; ++i) f[kPerDur + i] = 0.f;
            if (live) {
                const size_t c = ((size_t)m.b * (size_t)q.T + (size_t)t) * (size_t)q.U + (size_t)u;
                lse = q.lse[c];
                lo = p.lse_lo[c];
                const float *o = p.occ + c * (size_t)(q.D + 2);
                gb = o[0], gl = o[1];
#pragma unroll
                for (int i = 0; i < kTdtMaxD; ++i)
                    if (i < q.D) f[kPerDur + i] = scale * o[2 + i];
            }
            const float tot = gb + gl;
            mass = tot != 0.0f;  // (NaN: true)
            f[kLseV] = lse.x, f[kLoV] = lo.x, f[kLseD] = lse.y, f[kLoD] = lo.y;
            f[kCoef] = scale * tot, f[kGb] = scale * gb, f[kGl] = scale * gl;
        }
    }
    return __syncthreads_or(mass) != 0;
}

// h = tanh(enc[t] + pred[u]) of the tile's rows as binary16 hi / lo in LDS; zeros for rows that are not live (nothing is read
// for them).  After tj_rows; call, then __syncthreads().
__device__ __forceinline__ void tj_load_h(const TdtJointParams &p, const TJSmem &sm, const int b, const int t, const int ct) {
    const int J = p.J, J4 = J >> 2, ld = J + kTJPad;
    const TdtParams &q = p.lat;
    const float *erow = p.enc + ((size_t)b * (size_t)q.T + (size_t)t) * (size_t)J;
    for (int idx = threadIdx.x; idx < kTJRows * J4; idx += kTJThreads) {
        const int r = idx / J4, j = (idx - r * J4) * 4;
        tjh4 hi, lo;
        if (sm.row_live[r]) {
            const float4 e = *(const float4 *)(erow + j);
            const float4 c = *(const float4 *)(p.pred + ((size_t)b * (size_t)q.U + (size_t)(ct * kTJRows + r)) * (size_t)J + j);
            const float h[4] = {tj_tanh(e.x + c.x), tj_tanh(e.y + c.y), tj_tanh(e.z + c.z), tj_tanh(e.w + c.w)};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                tjf16 a, d;
                tj_split(h[k], a, d);
                hi[k] = a, lo[k] = d;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) hi[k] = (tjf16)0.f, lo[k] = (tjf16)0.f;
        }
        *(tjh4 *)(sm.hhi + r * ld + j) = hi;
        *(tjh4 *)(sm.hlo + r * ld + j) = lo;
    }
}

// the 8 elements W2[j0 ... j0 + 7][v] s2 of a B fragment (k = joint unit, column v on the lane); zeros for v >= V + D: no load
__device__ __forceinline__ void tj_w2_col(const TdtJointParams &p, const int j0, const int v, const float s2, tjh8 &hi, tjh8 &lo) {
    const int R = p.R;
    float w[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = v < R ? p.W2[(size_t)(j0 + e) * (size_t)R + v] : 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        tjf16 a, d;
        tj_split(w[e] * s2, a, d);
        hi[e] = a, lo[e] = d;
    }
}
// the 8 elements W2[j][v0 ... v0 + 7] s2 of a B fragment (k = logit column, joint unit j on the lane)
__device__ __forceinline__ void tj_w2_row(const TdtJointParams &p, const int j, const int v0, const float s2, tjh8 &hi, tjh8 &lo) {
    const int R = p.R;
    float w[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = v0 + e < R ? p.W2[(size_t)j * (size_t)R + v0 + e] : 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        tjf16 a, d;
        tj_split(w[e] * s2, a, d);
        hi[e] = a, lo[e] = d;
    }
}

// this wave's share of the J sum of the logits tile at columns v0 ... v0 + 31 -> part[wave]; then __syncthreads()
__device__ __forceinline__ void tj_logits_partial(const TdtJointParams &p, const TJSmem &sm, const int v0, const float s2) {
    const int J = p.J, ld = J + kTJPad;
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    tjf32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int ks = wave; ks < J / 16; ks += 4) {
        const int j0 = ks * 16 + half * 8;
        const tjh8 ahi = *(const tjh8 *)(sm.hhi + l31 * ld + j0);
        const tjh8 alo = *(const tjh8 *)(sm.hlo + l31 * ld + j0);
        tjh8 bhi, blo;
        tj_w2_col(p, j0, v0 + l31, s2, bhi, blo);
        acc = tj_mfma3(ahi, alo, bhi, blo, acc);
    }
    float *mine = sm.part + wave * kTJRows * kTJStage;
#pragma unroll
    for (int r = 0; r < 16; ++r) mine[tj_cd_row(r, half) * kTJStage + l31] = acc[r];
}

// logit (row, v0 + col) from the four partial tiles; -inf for a column beyond V + D (no load of b2 there)
__device__ __forceinline__ float tj_logit(const TdtJointParams &p, const TJSmem &sm, const int row, const int col, const int v0, const float w2inv) {
    const int v = v0 + col;
    if (v >= p.R) return -INFINITY;
    const int at = row * kTJStage + col;
    const float s = ((sm.part[at] + sm.part[kTJRows * kTJStage + at]) + sm.part[2 * kTJRows * kTJStage + at]) + sm.part[3 * kTJRows * kTJStage + at];
    return fmaf(s, w2inv, p.b2[v]);
}

// the merge of two (max, sum) pairs across lanes `off` apart; the lower lane's part first on both sides: the same bits in both
__device__ __forceinline__ void tj_merge(float &mx, float &s, const int j, const int off) {
    const float m2 = __shfl_xor(mx, off, 64), s2 = __shfl_xor(s, off, 64);
    const float nm = fmaxf(mx, m2);
    const float a = s * __expf(mx - nm), c = s2 * __expf(m2 - nm);
    s = (j & off) ? c + a : a + c;
    mx = nm;
}

// ---------------------------------------------------------------------------------------------
// Forward cell kernel: grid = B * T * CT, workgroup (b, t, ct)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTJThreads) tj_fwd_kernel(const TdtJointParams p) {
    extern __shared__ __attribute__((aligned(16))) char tj_sm[];
    const TdtParams &q = p.lat;
    const TJSmem sm = tj_carve(tj_sm, p.J);
    const int ct = blockIdx.x % p.CT, bt = blockIdx.x / p.CT;
    const int t = bt % q.T, b = bt / q.T;
    const TJUtt m = tj_utt(q, b);
    if (t >= m.Tb || ct * kTJRows > m.Lb) return;  // every row is padding
    tj_rows<false>(p, sm, m, t, ct, 0.f);
    tj_load_h(p, sm, b, t, ct);
    const float s2 = tj_w2_scale(p), w2inv = 1.0f / s2;
    __syncthreads();

    const int V = q.V, D = q.D;
    const int row = threadIdx.x >> 3, sub = threadIdx.x & 7;  // eight lanes per row, four columns of a tile each
    const int lab = sm.row_lab[row];
    float *f = sm.rowf + row * kTJRowF;
    float mv = kTJNegInit, sv = 0.f, md = kTJNegInit, sd = 0.f;
    for (int vt = 0; vt < p.vtiles; ++vt) {
        const int v0 = vt * kTJCols;
        tj_logits_partial(p, sm, v0, s2);
        __syncthreads();
        float x[4];
        float nv = mv, nd = md;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int v = v0 + sub * 4 + k;
            x[k] = tj_logit(p, sm, row, sub * 4 + k, v0, w2inv);  // (-inf beyond V + D)
            const bool tok = v < V;
            nv = tok ? fmaxf(nv, x[k]) : nv;
            nd = tok ? nd : fmaxf(nd, x[k]);
            // the 2 + D logits the edge weights need: every column is one thread's
            if (v == q.blank) f[kXb] = x[k];
            if (v == lab) f[kXl] = x[k];
            if (v >= V && v < p.R) f[kPerDur + v - V] = x[k];
        }
        float ev = 0.f, ed = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool tok = v0 + sub * 4 + k < V;
            const float e = __expf(x[k] - (tok ? nv : nd));
            ev += tok ? e : 0.f;
            ed += tok ? 0.f : e;
        }
        sv = sv * __expf(mv - nv) + ev;
        sd = sd * __expf(md - nd) + ed;
        mv = nv, md = nd;
        __syncthreads();  // the partial tiles are free again (and, after the last tile, the record is complete)
    }
#pragma unroll
    for (int off = 4; off >= 1; off >>= 1) {
        tj_merge(mv, sv, sub, off);
        tj_merge(md, sd, sub, off);
    }
    if (!sm.row_live[row]) return;  // live cells only
    const int u = ct * kTJRows + row;
    // lse = max + log(sum) as hi + lo: at logits of magnitude 10^3 an f32 lse alone is 1e-4 off, and the gradient pass's softmax
    // with it; the edge log-probabilities subtract the maximum first for the same reason
    const float logv = __logf(sv), logd = __logf(sd);
    const float lpb = ((f[kXb] - mv) - logv) - q.sigma;
    const float lpl = lab >= 0 ? ((f[kXl] - mv) - logv) - q.sigma : 0.0f;
    const size_t plane = (size_t)q.N * (size_t)q.Up;
    float *w = q.w + (size_t)b * (size_t)(2 * D) * plane + (size_t)(t + u) * (size_t)q.Up + u;
    if (sub < D) {  // D <= 8: lane i of the row's eight takes duration i
        const float ld = (f[kPerDur + sub] - md) - logd;
        w[(size_t)sub * plane] = lpb + ld;
        w[(size_t)(D + sub) * plane] = lpl + ld;
    }
    if (sub == 0) {
        const size_t c = ((size_t)b * (size_t)q.T + (size_t)t) * (size_t)q.U + (size_t)u;
        const float lseV = mv + logv, lseD = md + logd;
        q.lse[c] = make_float2(lseV, lseD);
        p.lse_lo[c] = make_float2(logv - (lseV - mv), logd - (lseD - md));
    }
}

// ---------------------------------------------------------------------------------------------
// Occupancy pass: one thread per lattice cell.  Edge 2 i is the blank edge, 2 i + 1 the label edge of duration i; its mass
//   e = exp(alpha(t,u) + w + beta(target) - ln P), 0 for an edge that does not exist.
// occ = {g_b, g_l, g_0 ... g_{D-1}}: the sums over the blank / label edges in the order of i, g_i = e(2 i) + e(2 i + 1).
// Exact zeros where no path crosses and for an utterance without a path; NaN for out-of-range lengths.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTJThreads) tj_occ_kernel(const TdtJointParams p) {
    const TdtParams &q = p.lat;
    const size_t c = (size_t)blockIdx.x * kTJThreads + threadIdx.x;
    if (c >= (size_t)q.B * (size_t)q.T * (size_t)q.U) return;
    const size_t bt = c / (size_t)q.U;
    const int u = (int)(c - bt * (size_t)q.U);
    const int b = (int)(bt / (size_t)q.T), t = (int)(bt - (size_t)b * (size_t)q.T);
    const TJUtt m = tj_utt(q, b);
    if (t >= m.Tb || u > m.Lb) return;  // padding: never read
    const int D = q.D;
    float *o = p.occ + c * (size_t)(D + 2);
    const float nan = __int_as_float(0x7fc00000);
    float gb = m.bad ? nan : 0.0f, gl = gb;
    const double lnP = q.lnP[b];  // NaN for out-of-range lengths, -inf without a path
    const int n = t + u;
    const size_t plane = (size_t)q.N * (size_t)q.Up;
    const size_t node = (size_t)b * plane + (size_t)n * (size_t)q.Up + u;
    const bool mass = !m.bad && lnP != -INFINITY;
    const double a = mass ? q.alpha[node] - lnP : -INFINITY;
    const float *w = q.w + (size_t)b * (size_t)(2 * D) * plane + (size_t)n * (size_t)q.Up + u;
#pragma unroll
    for (int i = 0; i < kTdtMaxD; ++i) {
        if (i < D) {
            const int d = q.dur[i];
            float eb = gb * 0.0f, el = eb;  // (NaN stays NaN)
            if (a != -INFINITY) {
                if (d > 0 && (t + d < m.Tb || (t + d == m.Tb && u == m.Lb)))
                    eb = __expf((float)(a + (double)w[(size_t)i * plane] + q.beta[node + (size_t)d * (size_t)q.Up]));  // (beta = -inf: 0)
                if (u < m.Lb && t + d < m.Tb)
                    el = __expf((float)(a + (double)w[(size_t)(D + i) * plane] + q.beta[node + (size_t)(d + 1) * (size_t)q.Up + 1]));
            }
            gb += eb, gl += el;
            o[2 + i] = eb + el;
        }
    }
    o[0] = gb, o[1] = gl;
}

// dlogits of this thread's four columns of the tile from their logits:
//   v < V:   coef softmax_tokens[v] - [v == blank] g_b - [v == label] g_l
//   v >= V:  coef softmax_durations[v - V] - g_{v - V}
// zeros for rows that are not live and for columns beyond V + D
__device__ __forceinline__ void tj_dlogits(const TdtJointParams &p, const TJSmem &sm, const int row, const int sub, const int v0,
                                           const float w2inv, float (&dl)[4]) {
    const bool live = sm.row_live[row] != 0;
    const float *f = sm.rowf + row * kTJRowF;
    const float lseV = f[kLseV], loV = f[kLoV], lseD = f[kLseD], loD = f[kLoD], coef = f[kCoef], gb = f[kGb], gl = f[kGl];
    const int lab = sm.row_lab[row];
    const int V = p.lat.V;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int v = v0 + sub * 4 + k;
        const float x = tj_logit(p, sm, row, sub * 4 + k, v0, w2inv);
        float g;
        if (v < V) {
            g = coef * __expf((x - lseV) - loV);
            g -= (v == p.lat.blank) ? gb : 0.0f;
            g -= (v == lab) ? gl : 0.0f;
        } else {
            g = coef * __expf((x - lseD) - loD) - f[kPerDur + min(v - V, kTdtMaxD - 1)];
        }
        dl[k] = (live && v < p.R) ? g : 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------
// Backward, part 1: dz = cost_scale (dlogits . W2^T) (1 - h^2) per live cell, summed in registers.
// grid = B * CT * NCH, workgroup (b, ct, chunk)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTJThreads) tj_bwd_dh_kernel(const TdtJointParams p) {
    extern __shared__ __attribute__((aligned(16))) char tj_sm[];
    const TdtParams &q = p.lat;
    const TJSmem sm = tj_carve(tj_sm, p.J);
    const int J = p.J, ld = J + kTJPad;
    const int chunk = blockIdx.x % p.NCH, rest = blockIdx.x / p.NCH;
    const int ct = rest % p.CT, b = rest / p.CT;
    const TJUtt m = tj_utt(q, b);
    const int t0 = chunk * kTJFrameChunk, t1 = min(t0 + kTJFrameChunk, m.Tb);
    if (t0 >= m.Tb || ct * kTJRows > m.Lb) return;
    if (!m.bad && q.lnP[b] == -INFINITY) return;  // no path: the reductions write its zeros without reading the partials
    const float s2 = tj_w2_scale(p), w2inv = 1.0f / s2;

    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const int njt = J / 32;
    constexpr int kMaxJt = kTJMaxJ / 32 / 4;  // column tiles of dh per wave
    const float cs = q.cost_scale ? q.cost_scale[b] : 1.0f;
    const float back = cs * (w2inv / kTJDlScale);
    tjf32x16 acc[kMaxJt], pacc[kMaxJt];
#pragma unroll
    for (int i = 0; i < kMaxJt; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) pacc[i][r] = 0.f;

    for (int t = t0; t < t1; ++t) {
        float *epart = p.encpart + (((size_t)b * (size_t)q.T + (size_t)t) * (size_t)p.CT + (size_t)ct) * (size_t)J;
        if (!tj_rows<true>(p, sm, m, t, ct, kTJDlScale)) {  // exactly zero mass on every row: dz = 0
            for (int j = threadIdx.x; j < J; j += kTJThreads) epart[j] = 0.f;
            __syncthreads();  // the rows are free again
            continue;
        }
        tj_load_h(p, sm, b, t, ct);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kMaxJt; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
        for (int vt = 0; vt < p.vtiles; ++vt) {
            const int v0 = vt * kTJCols;
            tj_logits_partial(p, sm, v0, s2);
            __syncthreads();
            float dl[4];
            tj_dlogits(p, sm, row, sub, v0, w2inv, dl);
            tjh4 hi, lo;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                tjf16 a, d;
                tj_split(dl[k], a, d);
                hi[k] = a, lo[k] = d;
            }
            *(tjh4 *)(sm.dlhi + row * kTJDlPad + sub * 4) = hi;
            *(tjh4 *)(sm.dllo + row * kTJDlPad + sub * 4) = lo;
            __syncthreads();
            // dh[rows][j] += dlogits[rows][v] W2[j][v]: A = dlogits (k = column), B = W2 rows of this wave's joint-unit tiles
#pragma unroll
            for (int i = 0; i < kMaxJt; ++i) {
                const int jt = wave + 4 * i;
                if (jt < njt) {
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        const int k0 = ks * 16 + half * 8;
                        const tjh8 ahi = *(const tjh8 *)(sm.dlhi + l31 * kTJDlPad + k0);
                        const tjh8 alo = *(const tjh8 *)(sm.dllo + l31 * kTJDlPad + k0);
                        tjh8 bhi, blo;
                        tj_w2_row(p, jt * 32 + l31, v0 + k0, s2, bhi, blo);
                        acc[i] = tj_mfma3(ahi, alo, bhi, blo, acc[i]);
                    }
                }
            }
            __syncthreads();  // the partial tiles and the dlogits tile are free again
        }
#pragma unroll
        for (int i = 0; i < kMaxJt; ++i) {
            const int jt = wave + 4 * i;
            if (jt < njt) {
                const int j = jt * 32 + l31;
                float dz[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rw = tj_cd_row(r, half);
                    const float h = (float)sm.hhi[rw * ld + j] + (float)sm.hlo[rw * ld + j];  // (0 for a row that is not live)
                    dz[r] = acc[i][r] * back * (1.0f - h * h);
                    pacc[i][r] += dz[r];
                }
                // the sum over the tile's rows in column order: rows 4 g ... 4 g + 3 are registers 4 (g / 2) ... of half g & 1, so the
                // running sum changes sides after every group
                float s = 0.f;
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    float mine = s;
#pragma unroll
                    for (int k = 0; k < 4; ++k) mine += dz[4 * (g >> 1) + k];
                    const float theirs = __shfl_xor(mine, 32, 64);
                    s = (half == (g & 1)) ? mine : theirs;
                }
                if (half == 0) epart[j] = s;
            }
        }
        __syncthreads();  // h and the rows are free again
    }
#pragma unroll
    for (int i = 0; i < kMaxJt; ++i) {
        const int jt = wave + 4 * i;
        if (jt < njt) {
            const int j = jt * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int u = ct * kTJRows + tj_cd_row(r, half);
                if (u > m.Lb) continue;  // not live: nothing is stored
                p.predpart[(((size_t)b * (size_t)p.NCH + (size_t)chunk) * (size_t)q.U + (size_t)u) * (size_t)J + j] = pacc[i][r];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The reductions of the dz partials.  One thread per four joint units.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTJThreads) tj_reduce_enc_kernel(const TdtJointParams p) {
    const TdtParams &q = p.lat;
    const int J4 = p.J >> 2;
    const size_t idx = (size_t)blockIdx.x * kTJThreads + threadIdx.x;
    if (idx >= (size_t)q.B * (size_t)q.T * (size_t)J4) return;
    const size_t bt = idx / J4;
    const int j = (int)(idx - bt * J4) * 4;
    const int b = (int)(bt / q.T), t = (int)(bt - (size_t)b * q.T);
    const TJUtt m = tj_utt(q, b);
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < m.Tb && (m.bad || q.lnP[b] != -INFINITY)) {
        for (int ct = 0; ct * kTJRows <= m.Lb; ++ct) {
            const float4 d = *(const float4 *)(p.encpart + (bt * (size_t)p.CT + (size_t)ct) * (size_t)p.J + j);
            sum.x += d.x, sum.y += d.y, sum.z += d.z, sum.w += d.w;
        }
    }
    *(float4 *)(p.d_enc + bt * (size_t)p.J + j) = sum;
}

__global__ void __launch_bounds__(kTJThreads) tj_reduce_pred_kernel(const TdtJointParams p) {
    const TdtParams &q = p.lat;
    const int J4 = p.J >> 2;
    const size_t idx = (size_t)blockIdx.x * kTJThreads + threadIdx.x;
    if (idx >= (size_t)q.B * (size_t)q.U * (size_t)J4) return;
    const size_t bu = idx / J4;
    const int j = (int)(idx - bu * J4) * 4;
    const int b = (int)(bu / q.U), u = (int)(bu - (size_t)b * q.U);
    const TJUtt m = tj_utt(q, b);
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
    if (u <= m.Lb && (m.bad || q.lnP[b] != -INFINITY)) {
        for (int c = 0; c * kTJFrameChunk < m.Tb; ++c) {
            const float4 d = *(const float4 *)(p.predpart + (((size_t)b * (size_t)p.NCH + (size_t)c) * (size_t)q.U + (size_t)u) * (size_t)p.J + j);
            sum.x += d.x, sum.y += d.y, sum.z += d.z, sum.w += d.w;
        }
    }
    *(float4 *)(p.d_pred + bu * (size_t)p.J + j) = sum;
}

// ---------------------------------------------------------------------------------------------
// Backward, part 2: the partial sums of dW2 = h^T . dlogits and db2 = column sums of dlogits, per (logit column tile, row chunk)
// ---------------------------------------------------------------------------------------------
// the power of two that puts 2 max |cost_scale| into [2^12, 2^13): one for the whole batch (dW2 sums over it).  NULL is a
// cost_scale of ones, bit for bit.
__device__ __forceinline__ float tj_batch_scale(const TdtParams &q) {
    if (!q.cost_scale) return 2048.0f;
    unsigned mbits = 0u;
    for (int i = threadIdx.x & 63; i < q.B; i += 64) mbits = max(mbits, __float_as_uint(q.cost_scale[i]) & 0x7fffffffu);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mbits = max(mbits, (unsigned)__shfl_xor((int)mbits, off, 64));
    const float x = __uint_as_float(mbits);
    if (!(x > 0.f) || !(x < 3.0e38f)) return 1.0f;
    return ldexpf(1.0f, min(12 - (ilogbf(x) + 1), kTJMaxScaleLog2));
}

__global__ void __launch_bounds__(kTJThreads) tj_bwd_dw_kernel(const TdtJointParams p) {
    extern __shared__ __attribute__((aligned(16))) char tj_sm[];
    const TdtParams &q = p.lat;
    const TJSmem sm = tj_carve(tj_sm, p.J);
    const int J = p.J, ld = J + kTJPad;
    const int vt = blockIdx.x % p.vtiles, chunk = blockIdx.x / p.vtiles;
    const int v0 = vt * kTJCols;
    const int vpad = p.vtiles * kTJCols;
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const int njt = J / 32;
    constexpr int kMaxJt = kTJMaxJ / 32 / 4;
    const float s2 = tj_w2_scale(p), w2inv = 1.0f / s2;
    const float G = tj_batch_scale(q);
    tjf32x16 acc[kMaxJt];
#pragma unroll
    for (int i = 0; i < kMaxJt; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    float bsum = 0.f;  // threads 0 ... 31: db2 of column v0 + thread

    const long long per_utt = (long long)q.T * p.CT;
    const long long total = (long long)q.B * per_utt;
    const long long first = (long long)chunk * p.tiles_per_chunk;
    const long long last = min(first + (long long)p.tiles_per_chunk, total);
    for (long long g = first; g < last; ++g) {
        const int b = (int)(g / per_utt), rem = (int)(g - (long long)b * per_utt);
        const int t = rem / p.CT, ct = rem - t * p.CT;
        const TJUtt m = tj_utt(q, b);
        if (t >= m.Tb || ct * kTJRows > m.Lb) continue;
        if (!m.bad && q.lnP[b] == -INFINITY) continue;
        const float cs = q.cost_scale ? q.cost_scale[b] : 1.0f;
        if (!tj_rows<true>(p, sm, m, t, ct, cs)) {  // exactly zero mass on every row: dlogits = 0
            __syncthreads();
            continue;
        }
        tj_load_h(p, sm, b, t, ct);
        __syncthreads();
        tj_logits_partial(p, sm, v0, s2);
        __syncthreads();
        float dl[4];
        tj_dlogits(p, sm, row, sub, v0, w2inv, dl);
        // the tile TRANSPOSED ([column][row]) for the B operand (k = row), and as it is for the column sums
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tjf16 a, d;
            tj_split(dl[k] * G, a, d);
            sm.dlhi[(sub * 4 + k) * kTJDlPad + row] = a;
            sm.dllo[(sub * 4 + k) * kTJDlPad + row] = d;
            sm.stage[row * kTJStage + sub * 4 + k] = dl[k];
        }
        __syncthreads();
        if (threadIdx.x < kTJCols) {
            float c = 0.f;
            for (int r = 0; r < kTJRows; ++r) c += sm.stage[r * kTJStage + threadIdx.x];
            bsum += c;
        }
        // dW2[j][v] += h[rows][j] dlogits[rows][v]: A = h^T (k = row), B = dlogits
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int k0 = ks * 16 + half * 8;
            const tjh8 bhi = *(const tjh8 *)(sm.dlhi + l31 * kTJDlPad + k0);
            const tjh8 blo = *(const tjh8 *)(sm.dllo + l31 * kTJDlPad + k0);
#pragma unroll
            for (int i = 0; i < kMaxJt; ++i) {
                const int jt = wave + 4 * i;
                if (jt < njt) {
                    const int j = jt * 32 + l31;
                    tjh8 ahi, alo;
#pragma unroll
                    for (int e = 0; e < 8; ++e) ahi[e] = sm.hhi[(k0 + e) * ld + j], alo[e] = sm.hlo[(k0 + e) * ld + j];
                    acc[i] = tj_mfma3(ahi, alo, bhi, blo, acc[i]);
                }
            }
        }
        __syncthreads();  // everything in LDS is free again
    }
    const float back = 1.0f / G;
#pragma unroll
    for (int i = 0; i < kMaxJt; ++i) {
        const int jt = wave + 4 * i;
        if (jt < njt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = jt * 32 + tj_cd_row(r, half);
                p.wpart[((size_t)chunk * (size_t)J + (size_t)j) * (size_t)vpad + v0 + l31] = acc[i][r] * back;
            }
        }
    }
    if (threadIdx.x < kTJCols) p.bpart[(size_t)chunk * (size_t)vpad + v0 + threadIdx.x] = bsum;
}

__global__ void __launch_bounds__(kTJThreads) tj_reduce_w_kernel(const TdtJointParams p) {
    const int R = p.R, J = p.J;
    const int vpad = p.vtiles * kTJCols;
    const size_t idx = (size_t)blockIdx.x * kTJThreads + threadIdx.x;
    const size_t nW = (size_t)J * (size_t)R;
    if (idx < nW) {
        const int j = (int)(idx / R), v = (int)(idx - (size_t)j * R);
        float s = 0.f;
        for (int c = 0; c < p.chunks; ++c) s += p.wpart[((size_t)c * (size_t)J + (size_t)j) * (size_t)vpad + v];
        p.dW2[idx] = s;
    } else if (idx < nW + (size_t)R) {
        const int v = (int)(idx - nW);
        float s = 0.f;
        for (int c = 0; c < p.chunks; ++c) s += p.bpart[(size_t)c * (size_t)vpad + v];
        p.db2[v] = s;
    }
}

// ---------------------------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------------------------
template <typename Kernel>
static hipError_t tj_set_lds(Kernel kernel, const size_t bytes) {  // per device and cheap: set before every launch
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

static uint32_t tj_blocks(const size_t n) { return (uint32_t)((n + kTJThreads - 1) / kTJThreads); }

static hipError_t launch_w2max(const TdtJointParams &p, hipStream_t s) {
    hipLaunchKernelGGL(tj_w2max_kernel, dim3(kTJAbsBlocks), dim3(kTJThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_tdt_joint_forward(const TdtJointParams &p, hipStream_t s) {
    hipError_t e = launch_w2max(p, s);
    if (e != hipSuccess) return e;
    const size_t lds = tj_smem_bytes(p.J);
    e = tj_set_lds(tj_fwd_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tj_fwd_kernel, dim3((uint32_t)p.lat.B * (uint32_t)p.lat.T * (uint32_t)p.CT), dim3(kTJThreads), lds, s, p);
    return hipGetLastError();
}

hipError_t launch_tdt_joint_backward(const TdtJointParams &p, const bool w2max_fresh, hipStream_t s) {
    const TdtParams &q = p.lat;
    hipError_t e = w2max_fresh ? hipSuccess : launch_w2max(p, s);  // (a forward of the same call has just left the entries)
    if (e != hipSuccess) return e;
    const size_t lds = tj_smem_bytes(p.J);
    e = tj_set_lds(tj_bwd_dh_kernel, lds);
    if (e != hipSuccess) return e;
    e = tj_set_lds(tj_bwd_dw_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tj_occ_kernel, dim3(tj_blocks((size_t)q.B * (size_t)q.T * (size_t)q.U)), dim3(kTJThreads), 0, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(tj_bwd_dh_kernel, dim3((uint32_t)q.B * (uint32_t)p.CT * (uint32_t)p.NCH), dim3(kTJThreads), lds, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(tj_reduce_enc_kernel, dim3(tj_blocks((size_t)q.B * (size_t)q.T * (size_t)(p.J / 4))), dim3(kTJThreads), 0, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(tj_reduce_pred_kernel, dim3(tj_blocks((size_t)q.B * (size_t)q.U * (size_t)(p.J / 4))), dim3(kTJThreads), 0, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(tj_bwd_dw_kernel, dim3((uint32_t)p.vtiles * (uint32_t)p.chunks), dim3(kTJThreads), lds, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(tj_reduce_w_kernel, dim3(tj_blocks((size_t)p.J * (size_t)p.R + (size_t)p.R)), dim3(kTJThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace rnnt
