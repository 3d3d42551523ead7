// rnnt_pruned_joint_kernels.hip -- the fused joint on the pruned band: costs and the four gradients from the projections, without
// the band's logits [B, T, S, V] or the gathered prediction rows [B, T, S, J] ever existing in memory (include/rnnt_pruned_joint.h;
// rnnt_pruned_joint.h for the workspace).  The lattice sweeps are rnnt_pruned_kernels.hip's, unchanged.
//
//   pj_w2max_kernel      abs-max of W2 in 64 per-block entries: the power of two s2 that puts max |s2 W2| into [2^13, 2^14)
//   pj_fwd_kernel        a workgroup = 32 consecutive band slots of one utterance.  h = tanh(enc[t] + pred[u]) is formed in the
//                        loader, behind the presence test (an absent slot forms no address at all), and kept in LDS as binary16
//                        hi + lo.  The logits exist 32 columns at a time: the four waves split the J sum of a 32 x 32 tile
//                        (hi.hi + lo.hi + hi.lo on v_mfma_f32_32x32x16_f16, f32 accumulation), the partial tiles meet in LDS
//                        and eight lanes per row carry the online log-softmax across the tiles.  Stores {lpb, lpl} and lse.
//   pj_bwd_dh_kernel     the same tile loop; per tile: dlogits from alpha / edge / lnP / lse (unit cost_scale, scaled by 2^12
//                        and split), dh += dlogits . W2^T on the MFMAs (a wave owns J / 32 / 4 column tiles of dh), at the end
//                        dz = cost_scale dh (1 - h^2) per present slot.
//   pj_reduce_enc_kernel d_enc_proj[b, t] = sum over s of dz, in slot order; zeros for t >= T_b
//   pj_reduce_pred_kernel d_pred_proj[b, u] = sum over the frames whose band holds u, in frame order (a scan with the range test:
//                        s_begin need not be monotone); zeros for rows no present cell points at
//   pj_bwd_dw_kernel     workgroup (vocabulary tile, row chunk): recomputes h and the tile's logits for every row tile of its
//                        chunk, dW2 partial += h^T . dlogits on the MFMAs (dlogits carry cost_scale and one power of two for the
//                        whole batch), db2 partial = column sums; one partial per chunk
//   pj_reduce_w_kernel   dW2 / db2 = the partials summed in chunk order
//
// No atomics, no memset; every sum has an order fixed by the shapes, and an utterance's tiles hold that utterance's rows alone:
// costs, d_enc_proj and d_pred_proj of an utterance do not depend on the batch around it.
//
// THE RANGE TEST COMES FIRST.  pj_row() is the only place a slot's (t, u) is formed; u is a 64-bit sum, and no address into
// enc_proj, pred_proj, the labels or the lattice arrays is formed for a row whose `present` is false.
#include "rnnt_pruned_joint.h"

#include <math.h>

namespace rnnt {

typedef _Float16 pjf16;
typedef _Float16 pjh4 __attribute__((ext_vector_type(4)));
typedef _Float16 pjh8 __attribute__((ext_vector_type(8)));
typedef float pjf32x16 __attribute__((ext_vector_type(16)));

constexpr int kPJThreads = 256;           // four waves
constexpr int kPJPad = 8;                 // binary16 elements of padding per h row: rows stay 16-byte aligned
constexpr int kPJStage = 33;              // row stride of the f32 staging tiles
constexpr int kPJDlPad = 40;              // row stride (binary16) of the dlogits tiles: 80 bytes, 16-byte aligned
constexpr float kPJNegInit = -3.0e38f;    // finite: lanes without columns merge to (this, 0), not to NaN
constexpr float kPJDlScale = 4096.0f;     // unit-scale dlogits (|.| <= 2) times 2^12 before the binary16 split
constexpr int kPJW2Log2 = 14;             // max |s2 W2| < 2^14
constexpr int kPJMaxScaleLog2 = 100;      // no power-of-two scale beyond 2^100 (operands below 2^-86: the scale stops growing)

// row of accumulator register `reg` in a 32 x 32 result (the column is lane & 31)
__device__ __forceinline__ constexpr int pj_cd_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

__device__ __forceinline__ void pj_split(const float x, pjf16 &hi, pjf16 &lo) {
    hi = (pjf16)x;
    lo = (pjf16)(x - (float)hi);
}

__device__ __forceinline__ pjf32x16 pj_mfma3(const pjh8 ahi, const pjh8 alo, const pjh8 bhi, const pjh8 blo, pjf32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, bhi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, bhi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, blo, acc, 0, 0, 0);
    return acc;
}

// tanh(x) = sign(x) (1 - 2 / (1 + e^{2|x|})): saturates at +-inf.  On |x| the quotient is at most 1 and shrinks as h saturates,
// so the absolute error stays below ~1e-7 on both sides (1 - 2 / (1 + e^{2x}) on a negative x rounds a quotient near 2: 4e-7,
// and W2 multiplies that).  The exponent 2|x| log2(e) is formed as hi + lo (the product's rounding error would otherwise be a
// relative error of e^{2|x|} of 6e-8 times the exponent).
__device__ __forceinline__ float pj_tanh(const float x) {
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
__global__ void __launch_bounds__(kPJThreads) pj_w2max_kernel(const PrunedJointParams p) {
    extern __shared__ __attribute__((aligned(16))) char pj_sm[];
    unsigned *red = (unsigned *)pj_sm;
    const size_t n = (size_t)p.J * (size_t)p.band.V;
    unsigned m = 0u;
    for (size_t i = (size_t)blockIdx.x * kPJThreads + threadIdx.x; i < n; i += (size_t)kPJAbsBlocks * kPJThreads)
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
// The exponent stops at kPJMaxScaleLog2: s2 and 1 / s2 stay normal numbers for a max |W2| down to the smallest subnormal.
// Every wave of a consumer redoes this: one entry per lane.
__device__ __forceinline__ float pj_w2_scale(const PrunedJointParams &p) {
    unsigned m = __hip_atomic_load(p.w2max + (threadIdx.x & 63), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
    const float x = __uint_as_float(m);
    if (!(x > 0.f) || !(x < 3.0e38f)) return 1.0f;
    return ldexpf(1.0f, min(kPJW2Log2 - (ilogbf(x) + 1), kPJMaxScaleLog2));
}

// ---------------------------------------------------------------------------------------------
// The rows of a tile.
// ---------------------------------------------------------------------------------------------
struct PJUtt {
    int b, Tb, Lb;
    bool bad;
};

__device__ __forceinline__ PJUtt pj_utt(const PrunedParams &q, const int b) {
    PJUtt m;
    m.b = b;
    const int Tb = q.input_lengths[b], Lb = q.label_lengths[b];
    m.bad = Tb < 1 || Tb > q.T || Lb < 0 || Lb > q.U - 1;
    m.Tb = min(max(Tb, 1), q.T);
    m.Lb = min(max(Lb, 0), q.U - 1);
    return m;
}

struct PJRow {
    int t;        // frame of the slot (valid slots only)
    int u;        // lattice column, -1 for an absent slot
    uint32_t c;   // slot index in the [B][T][S] arrays
};

// slot `slot` of utterance m.b (slot = t S + s).  The range test: everything else looks at r.u >= 0 only.
__device__ __forceinline__ PJRow pj_row(const PrunedParams &q, const PJUtt &m, const long long slot) {
    PJRow r;
    r.t = 0, r.u = -1, r.c = 0u;
    if (slot >= (long long)q.T * q.S) return r;
    const int t = (int)(slot / q.S), s = (int)(slot - (long long)t * q.S);
    r.t = t;
    r.c = (uint32_t)((long long)m.b * q.T * q.S + slot);
    if (t >= m.Tb) return r;
    const long long u = (long long)q.s_begin[(size_t)m.b * (size_t)q.T + (size_t)t] + (long long)s;
    if (u >= 0 && u <= (long long)m.Lb) r.u = (int)u;
    return r;
}

// LDS carve (bytes), shared by the three tile kernels
struct PJSmem {
    pjf16 *hhi, *hlo;  // [32][J + 8]
    float *part;       // [4][32][33]: the waves' partial logits tiles
    float *stage;      // [32][33]
    pjf16 *dlhi, *dllo;  // [32][40]
    int *row_u, *row_t, *row_lab;  // [32]
    float *row_lse, *row_lse2, *row_coef, *row_eb, *row_el;  // [32]
};
__host__ __device__ inline size_t pj_smem_bytes(const int J) {
    return (size_t)2 * kPJRows * (J + kPJPad) * 2 + (size_t)4 * kPJRows * kPJStage * 4 + (size_t)kPJRows * kPJStage * 4 +
           (size_t)2 * kPJRows * kPJDlPad * 2 + (size_t)8 * kPJRows * 4;
}
__device__ __forceinline__ PJSmem pj_carve(char *sm, const int J) {
    PJSmem s;
    s.hhi = (pjf16 *)sm;
    s.hlo = s.hhi + kPJRows * (J + kPJPad);
    s.part = (float *)(s.hlo + kPJRows * (J + kPJPad));
    s.stage = s.part + 4 * kPJRows * kPJStage;
    s.dlhi = (pjf16 *)(s.stage + kPJRows * kPJStage);
    s.dllo = s.dlhi + kPJRows * kPJDlPad;
    s.row_u = (int *)(s.dllo + kPJRows * kPJDlPad);
    s.row_t = s.row_u + kPJRows;
    s.row_lab = s.row_t + kPJRows;
    s.row_lse = (float *)(s.row_lab + kPJRows);
    s.row_lse2 = s.row_lse + kPJRows;
    s.row_coef = s.row_lse2 + kPJRows;
    s.row_eb = s.row_coef + kPJRows;
    s.row_el = s.row_eb + kPJRows;
    return s;
}

// threads 0 ... 31: the tile's rows (and, for the gradient kernels, what dlogits needs of each).  `scale` multiplies the three
// dlogits coefficients.  Call, then __syncthreads().
template <bool GRAD>
__device__ __forceinline__ void pj_rows(const PrunedJointParams &p, const PJSmem &sm, const PJUtt &m, const int tile, const float scale) {
    const PrunedParams &q = p.band;
    const int r = threadIdx.x;
    if (r >= kPJRows) return;
    const PJRow row = pj_row(q, m, (long long)tile * kPJRows + r);
    sm.row_u[r] = row.u;
    sm.row_t[r] = row.t;
    int lab = -1;
    if (row.u >= 0 && row.u < m.Lb) {
        lab = q.labels[(size_t)m.b * (size_t)(q.U - 1) + (size_t)row.u];
        lab = min(max(lab, 0), q.V - 1);
    }
    sm.row_lab[r] = lab;
    if constexpr (GRAD) {
        float lse = 0.f, lse2 = 0.f, eb = 0.f, el = 0.f;
        if (row.u >= 0) {
            const double lnP = q.lnP[m.b];
            const double a = q.alpha[row.c];
            const double2 ed = q.edge[row.c];
            lse = q.lse[row.c];
            lse2 = p.lse_lo[row.c];
            eb = __expf((float)(a + ed.x - lnP));  // (-inf: 0)
            if (lab >= 0) el = __expf((float)(a + ed.y - lnP));
            if (m.bad) eb = el = __int_as_float(0x7fc00000);
        }
        sm.row_lse[r] = lse;
        sm.row_lse2[r] = lse2;
        sm.row_coef[r] = scale * (eb + el + q.fe_lambda * el);
        sm.row_eb[r] = scale * eb;
        sm.row_el[r] = scale * ((1.0f + q.fe_lambda) * el);
    }
}

// h = tanh(enc[t] + pred[u]) of the tile's rows as binary16 hi / lo in LDS; zeros for absent rows (nothing is read for them).
// After pj_rows + barrier; call, then __syncthreads().
__device__ __forceinline__ void pj_load_h(const PrunedJointParams &p, const PJSmem &sm, const int b) {
    const int J = p.J, J4 = J >> 2, ld = J + kPJPad;
    const PrunedParams &q = p.band;
    for (int idx = threadIdx.x; idx < kPJRows * J4; idx += kPJThreads) {
        const int r = idx / J4, j = (idx - r * J4) * 4;
        const int u = sm.row_u[r];
        pjh4 hi, lo;
        if (u >= 0) {
            const float4 e = *(const float4 *)(p.enc + ((size_t)b * (size_t)q.T + (size_t)sm.row_t[r]) * (size_t)J + j);
            const float4 c = *(const float4 *)(p.pred + ((size_t)b * (size_t)q.U + (size_t)u) * (size_t)J + j);
            const float h[4] = {pj_tanh(e.x + c.x), pj_tanh(e.y + c.y), pj_tanh(e.z + c.z), pj_tanh(e.w + c.w)};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                pjf16 a, d;
                pj_split(h[k], a, d);
                hi[k] = a, lo[k] = d;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) hi[k] = (pjf16)0.f, lo[k] = (pjf16)0.f;
        }
        *(pjh4 *)(sm.hhi + r * ld + j) = hi;
        *(pjh4 *)(sm.hlo + r * ld + j) = lo;
    }
}

// the 8 elements W2[j0 ... j0 + 7][v] s2 of a B fragment (k = joint unit, column v on the lane); zeros for v >= V: no load
__device__ __forceinline__ void pj_w2_col(const PrunedJointParams &p, const int j0, const int v, const float s2, pjh8 &hi, pjh8 &lo) {
    const int V = p.band.V;
    float w[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = v < V ? p.W2[(size_t)(j0 + e) * (size_t)V + v] : 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        pjf16 a, d;
        pj_split(w[e] * s2, a, d);
        hi[e] = a, lo[e] = d;
    }
}
// the 8 elements W2[j][v0 ... v0 + 7] s2 of a B fragment (k = vocabulary column, joint unit j on the lane)
__device__ __forceinline__ void pj_w2_row(const PrunedJointParams &p, const int j, const int v0, const float s2, pjh8 &hi, pjh8 &lo) {
    const int V = p.band.V;
    float w[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = v0 + e < V ? p.W2[(size_t)j * (size_t)V + v0 + e] : 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        pjf16 a, d;
        pj_split(w[e] * s2, a, d);
        hi[e] = a, lo[e] = d;
    }
}

// this wave's share of the J sum of the logits tile at columns v0 ... v0 + 31 -> part[wave]; then __syncthreads()
__device__ __forceinline__ void pj_logits_partial(const PrunedJointParams &p, const PJSmem &sm, const int v0, const float s2) {
    const int J = p.J, ld = J + kPJPad;
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    pjf32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int ks = wave; ks < J / 16; ks += 4) {
        const int j0 = ks * 16 + half * 8;
        const pjh8 ahi = *(const pjh8 *)(sm.hhi + l31 * ld + j0);
        const pjh8 alo = *(const pjh8 *)(sm.hlo + l31 * ld + j0);
        pjh8 bhi, blo;
        pj_w2_col(p, j0, v0 + l31, s2, bhi, blo);
        acc = pj_mfma3(ahi, alo, bhi, blo, acc);
    }
    float *mine = sm.part + wave * kPJRows * kPJStage;
#pragma unroll
    for (int r = 0; r < 16; ++r) mine[pj_cd_row(r, half) * kPJStage + l31] = acc[r];
}

// logit (row, v0 + col) from the four partial tiles; -inf for a column beyond V (no load of b2 there)
__device__ __forceinline__ float pj_logit(const PrunedJointParams &p, const PJSmem &sm, const int row, const int col, const int v0, const float w2inv) {
    const int v = v0 + col;
    if (v >= p.band.V) return -INFINITY;
    const int at = row * kPJStage + col;
    const float s = ((sm.part[at] + sm.part[kPJRows * kPJStage + at]) + sm.part[2 * kPJRows * kPJStage + at]) + sm.part[3 * kPJRows * kPJStage + at];
    return fmaf(s, w2inv, p.b2[v]);
}

// ---------------------------------------------------------------------------------------------
// Forward cell kernel
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPJThreads) pj_fwd_kernel(const PrunedJointParams p) {
    extern __shared__ __attribute__((aligned(16))) char pj_sm[];
    const PrunedParams &q = p.band;
    const PJSmem sm = pj_carve(pj_sm, p.J);
    const int b = blockIdx.x / p.tiles_per_utt, tile = blockIdx.x - b * p.tiles_per_utt;
    const PJUtt m = pj_utt(q, b);
    if ((long long)tile * kPJRows >= (long long)m.Tb * q.S) return;  // every row is a padded frame
    pj_rows<false>(p, sm, m, tile, 0.f);
    __syncthreads();
    pj_load_h(p, sm, b);
    const float s2 = pj_w2_scale(p), w2inv = 1.0f / s2;
    __syncthreads();

    const int row = threadIdx.x >> 3, sub = threadIdx.x & 7;  // eight lanes per row, four columns of a tile each
    const int lab = sm.row_lab[row];
    float mx = kPJNegInit, ssum = 0.f, xb = -INFINITY, xl = -INFINITY;
    for (int vt = 0; vt < p.vtiles; ++vt) {
        const int v0 = vt * kPJCols;
        pj_logits_partial(p, sm, v0, s2);
        __syncthreads();
        float x[4];
        float nm = mx;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x[k] = pj_logit(p, sm, row, sub * 4 + k, v0, w2inv);
            nm = fmaxf(nm, x[k]);
            const int v = v0 + sub * 4 + k;
            if (v == q.blank) xb = x[k];
            if (v == lab) xl = x[k];
        }
        float e = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) e += __expf(x[k] - nm);
        ssum = ssum * __expf(mx - nm) + e;
        mx = nm;
        __syncthreads();  // the partial tiles are free again
    }
#pragma unroll
    for (int off = 4; off >= 1; off >>= 1) {
        const float m2 = __shfl_xor(mx, off, 64), s2b = __shfl_xor(ssum, off, 64);
        const float nm = fmaxf(mx, m2);
        const float a = ssum * __expf(mx - nm), c = s2b * __expf(m2 - nm);
        ssum = (sub & off) ? c + a : a + c;  // lower lane's part first on both sides: the pair ends with the same bits
        mx = nm;
        xb = fmaxf(xb, __shfl_xor(xb, off, 64));
        xl = fmaxf(xl, __shfl_xor(xl, off, 64));
    }
    if (sub != 0 || sm.row_u[row] < 0) return;  // present slots only
    const PJRow r = pj_row(q, m, (long long)tile * kPJRows + row);
    // lse = mx + log(sum) as hi + lo: at logits of magnitude 10^3 an f32 lse alone is 1e-4 off, and the gradient pass's softmax
    // with it; the edge log-probabilities subtract mx first for the same reason
    const float logs = __logf(ssum);
    const float lse = mx + logs;
    float2 out;
    out.x = (xb - mx) - logs;
    out.y = lab >= 0 ? (xl - mx) - logs : 0.0f;
    q.lp[r.c] = out;
    q.lse[r.c] = lse;
    p.lse_lo[r.c] = logs - (lse - mx);
}

// dlogits of this thread's four columns of the tile from their logits: coef softmax - [blank] eb - [label] el; zeros for absent
// rows and for columns beyond V
__device__ __forceinline__ void pj_dlogits(const PrunedJointParams &p, const PJSmem &sm, const int row, const int sub, const int v0,
                                           const float w2inv, float (&dl)[4]) {
    const bool present = sm.row_u[row] >= 0;
    const float lse = sm.row_lse[row], lse2 = sm.row_lse2[row], coef = sm.row_coef[row], eb = sm.row_eb[row], el = sm.row_el[row];
    const int lab = sm.row_lab[row];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int v = v0 + sub * 4 + k;
        const float x = pj_logit(p, sm, row, sub * 4 + k, v0, w2inv);
        float g = coef * __expf((x - lse) - lse2);
        g -= (v == p.band.blank) ? eb : 0.0f;
        g -= (v == lab) ? el : 0.0f;
        dl[k] = (present && v < p.band.V) ? g : 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------
// Backward, part 1: dz = cost_scale (dlogits . W2^T) (1 - h^2) per present slot
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPJThreads) pj_bwd_dh_kernel(const PrunedJointParams p) {
    extern __shared__ __attribute__((aligned(16))) char pj_sm[];
    const PrunedParams &q = p.band;
    const PJSmem sm = pj_carve(pj_sm, p.J);
    const int J = p.J, ld = J + kPJPad;
    const int b = blockIdx.x / p.tiles_per_utt, tile = blockIdx.x - b * p.tiles_per_utt;
    const PJUtt m = pj_utt(q, b);
    if ((long long)tile * kPJRows >= (long long)m.Tb * q.S) return;
    if (!m.bad && q.lnP[b] == -INFINITY) return;  // no path: the reductions write its zeros without reading dz
    pj_rows<true>(p, sm, m, tile, kPJDlScale);
    __syncthreads();
    pj_load_h(p, sm, b);
    const float s2 = pj_w2_scale(p), w2inv = 1.0f / s2;
    __syncthreads();

    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const int njt = J / 32;
    constexpr int kMaxJt = kPJMaxJ / 32 / 4;  // column tiles of dh per wave
    pjf32x16 acc[kMaxJt];
#pragma unroll
    for (int i = 0; i < kMaxJt; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    for (int vt = 0; vt < p.vtiles; ++vt) {
        const int v0 = vt * kPJCols;
        pj_logits_partial(p, sm, v0, s2);
        __syncthreads();
        float dl[4];
        pj_dlogits(p, sm, row, sub, v0, w2inv, dl);
        pjh4 hi, lo;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pjf16 a, d;
            pj_split(dl[k], a, d);
            hi[k] = a, lo[k] = d;
        }
        *(pjh4 *)(sm.dlhi + row * kPJDlPad + sub * 4) = hi;
        *(pjh4 *)(sm.dllo + row * kPJDlPad + sub * 4) = lo;
        __syncthreads();
        // dh[rows][j] += dlogits[rows][v] W2[j][v]: A = dlogits (k = column), B = W2 rows of this wave's joint-unit tiles
#pragma unroll
        for (int i = 0; i < kMaxJt; ++i) {
            const int jt = wave + 4 * i;
            if (jt < njt) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const int k0 = ks * 16 + half * 8;
                    const pjh8 ahi = *(const pjh8 *)(sm.dlhi + l31 * kPJDlPad + k0);
                    const pjh8 alo = *(const pjh8 *)(sm.dllo + l31 * kPJDlPad + k0);
                    pjh8 bhi, blo;
                    pj_w2_row(p, jt * 32 + l31, v0 + k0, s2, bhi, blo);
                    acc[i] = pj_mfma3(ahi, alo, bhi, blo, acc[i]);
                }
            }
        }
        __syncthreads();  // the partial tiles and the dlogits tile are free again
    }
    const float cs = q.cost_scale ? q.cost_scale[b] : 1.0f;
    const float back = cs * (w2inv / kPJDlScale);
#pragma unroll
    for (int i = 0; i < kMaxJt; ++i) {
        const int jt = wave + 4 * i;
        if (jt < njt) {
            const int j = jt * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rw = pj_cd_row(r, half);
                if (sm.row_u[rw] < 0) continue;  // absent: nothing is stored
                const float h = (float)sm.hhi[rw * ld + j] + (float)sm.hlo[rw * ld + j];
                const size_t c = (size_t)b * (size_t)q.T * (size_t)q.S + (size_t)tile * kPJRows + (size_t)rw;
                p.dz[c * (size_t)J + j] = acc[i][r] * back * (1.0f - h * h);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The reductions of dz.  One thread per four joint units.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPJThreads) pj_reduce_enc_kernel(const PrunedJointParams p) {
    const PrunedParams &q = p.band;
    const int J4 = p.J >> 2;
    const size_t idx = (size_t)blockIdx.x * kPJThreads + threadIdx.x;
    if (idx >= (size_t)q.B * (size_t)q.T * (size_t)J4) return;
    const size_t bt = idx / J4;
    const int j = (int)(idx - bt * J4) * 4;
    const int b = (int)(bt / q.T), t = (int)(bt - (size_t)b * q.T);
    const PJUtt m = pj_utt(q, b);
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < m.Tb && (m.bad || q.lnP[b] != -INFINITY)) {
        for (int s = 0; s < q.S; ++s) {
            const PJRow r = pj_row(q, m, (long long)t * q.S + s);
            if (r.u < 0) continue;
            const float4 d = *(const float4 *)(p.dz + (size_t)r.c * (size_t)p.J + j);
            sum.x += d.x, sum.y += d.y, sum.z += d.z, sum.w += d.w;
        }
    }
    *(float4 *)(p.d_enc + bt * (size_t)p.J + j) = sum;
}

// a workgroup per (b, u): the scan over the frames is shared by its threads
__global__ void __launch_bounds__(kPJThreads) pj_reduce_pred_kernel(const PrunedJointParams p) {
    const PrunedParams &q = p.band;
    const int J4 = p.J >> 2;
    const int b = blockIdx.x / q.U, u = blockIdx.x - b * q.U;
    if ((int)threadIdx.x >= J4) return;
    const int j = threadIdx.x * 4;
    const PJUtt m = pj_utt(q, b);
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
    if (u <= m.Lb && (m.bad || q.lnP[b] != -INFINITY)) {
        const int *sbp = q.s_begin + (size_t)b * (size_t)q.T;
        for (int t = 0; t < m.Tb; ++t) {
            const long long s = (long long)u - (long long)sbp[t];
            if (s < 0 || s >= (long long)q.S) continue;
            const size_t c = ((size_t)b * (size_t)q.T + (size_t)t) * (size_t)q.S + (size_t)s;
            const float4 d = *(const float4 *)(p.dz + c * (size_t)p.J + j);
            sum.x += d.x, sum.y += d.y, sum.z += d.z, sum.w += d.w;
        }
    }
    *(float4 *)(p.d_pred + ((size_t)b * (size_t)q.U + (size_t)u) * (size_t)p.J + j) = sum;
}

// ---------------------------------------------------------------------------------------------
// Backward, part 2: the partial sums of dW2 = h^T . dlogits and db2 = column sums of dlogits, per (vocabulary tile, row chunk)
// ---------------------------------------------------------------------------------------------
// the power of two that puts 2 max |cost_scale| into [2^12, 2^13): one for the whole batch (dW2 sums over it).  NULL is a
// cost_scale of ones, bit for bit.
__device__ __forceinline__ float pj_batch_scale(const PrunedParams &q) {
    if (!q.cost_scale) return 2048.0f;
    unsigned mbits = 0u;
    for (int i = threadIdx.x & 63; i < q.B; i += 64) mbits = max(mbits, __float_as_uint(q.cost_scale[i]) & 0x7fffffffu);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mbits = max(mbits, (unsigned)__shfl_xor((int)mbits, off, 64));
    const float x = __uint_as_float(mbits);
    if (!(x > 0.f) || !(x < 3.0e38f)) return 1.0f;
    return ldexpf(1.0f, min(12 - (ilogbf(x) + 1), kPJMaxScaleLog2));
}

__global__ void __launch_bounds__(kPJThreads) pj_bwd_dw_kernel(const PrunedJointParams p) {
    extern __shared__ __attribute__((aligned(16))) char pj_sm[];
    const PrunedParams &q = p.band;
    const PJSmem sm = pj_carve(pj_sm, p.J);
    const int J = p.J, ld = J + kPJPad;
    const int vt = blockIdx.x % p.vtiles, chunk = blockIdx.x / p.vtiles;
    const int v0 = vt * kPJCols;
    const int vpad = p.vtiles * kPJCols;
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const int njt = J / 32;
    constexpr int kMaxJt = kPJMaxJ / 32 / 4;
    const float s2 = pj_w2_scale(p), w2inv = 1.0f / s2;
    const float G = pj_batch_scale(q);
    pjf32x16 acc[kMaxJt];
#pragma unroll
    for (int i = 0; i < kMaxJt; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    float bsum = 0.f;  // threads 0 ... 31: db2 of column v0 + thread

    const long long total = (long long)q.B * p.tiles_per_utt;
    const long long first = (long long)chunk * p.tiles_per_chunk;
    const long long last = min(first + (long long)p.tiles_per_chunk, total);
    for (long long g = first; g < last; ++g) {
        const int b = (int)(g / p.tiles_per_utt), tile = (int)(g - (long long)b * p.tiles_per_utt);
        const PJUtt m = pj_utt(q, b);
        if ((long long)tile * kPJRows >= (long long)m.Tb * q.S) continue;
        if (!m.bad && q.lnP[b] == -INFINITY) continue;
        const float cs = q.cost_scale ? q.cost_scale[b] : 1.0f;
        pj_rows<true>(p, sm, m, tile, cs);
        __syncthreads();
        pj_load_h(p, sm, b);
        __syncthreads();
        pj_logits_partial(p, sm, v0, s2);
        __syncthreads();
        float dl[4];
        pj_dlogits(p, sm, row, sub, v0, w2inv, dl);
        // the tile TRANSPOSED ([column][row]) for the B operand (k = row), and as it is for the column sums
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pjf16 a, d;
            pj_split(dl[k] * G, a, d);
            sm.dlhi[(sub * 4 + k) * kPJDlPad + row] = a;
            sm.dllo[(sub * 4 + k) * kPJDlPad + row] = d;
            sm.stage[row * kPJStage + sub * 4 + k] = dl[k];
        }
        __syncthreads();
        if (threadIdx.x < kPJCols) {
            float c = 0.f;
            for (int r = 0; r < kPJRows; ++r) c += sm.stage[r * kPJStage + threadIdx.x];
            bsum += c;
        }
        // dW2[j][v] += h[rows][j] dlogits[rows][v]: A = h^T (k = row), B = dlogits
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int k0 = ks * 16 + half * 8;
            const pjh8 bhi = *(const pjh8 *)(sm.dlhi + l31 * kPJDlPad + k0);
            const pjh8 blo = *(const pjh8 *)(sm.dllo + l31 * kPJDlPad + k0);
#pragma unroll
            for (int i = 0; i < kMaxJt; ++i) {
                const int jt = wave + 4 * i;
                if (jt < njt) {
                    const int j = jt * 32 + l31;
                    pjh8 ahi, alo;
#pragma unroll
                    for (int e = 0; e < 8; ++e) ahi[e] = sm.hhi[(k0 + e) * ld + j], alo[e] = sm.hlo[(k0 + e) * ld + j];
                    acc[i] = pj_mfma3(ahi, alo, bhi, blo, acc[i]);
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
                const int j = jt * 32 + pj_cd_row(r, half);
                p.wpart[((size_t)chunk * (size_t)J + (size_t)j) * (size_t)vpad + v0 + l31] = acc[i][r] * back;
            }
        }
    }
    if (threadIdx.x < kPJCols) p.bpart[(size_t)chunk * (size_t)vpad + v0 + threadIdx.x] = bsum;
}

__global__ void __launch_bounds__(kPJThreads) pj_reduce_w_kernel(const PrunedJointParams p) {
    const int V = p.band.V, J = p.J;
    const int vpad = p.vtiles * kPJCols;
    const size_t idx = (size_t)blockIdx.x * kPJThreads + threadIdx.x;
    const size_t nW = (size_t)J * (size_t)V;
    if (idx < nW) {
        const int j = (int)(idx / V), v = (int)(idx - (size_t)j * V);
        float s = 0.f;
        for (int c = 0; c < p.chunks; ++c) s += p.wpart[((size_t)c * (size_t)J + (size_t)j) * (size_t)vpad + v];
        p.dW2[idx] = s;
    } else if (idx < nW + (size_t)V) {
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
static hipError_t pj_set_lds(Kernel kernel, const size_t bytes) {  // per device and cheap: set before every launch
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

static hipError_t launch_w2max(const PrunedJointParams &p, hipStream_t s) {
    hipLaunchKernelGGL(pj_w2max_kernel, dim3(kPJAbsBlocks), dim3(kPJThreads), 16, s, p);
    return hipGetLastError();
}

hipError_t launch_pruned_joint_forward(const PrunedJointParams &p, hipStream_t s) {
    hipError_t e = launch_w2max(p, s);
    if (e != hipSuccess) return e;
    const size_t lds = pj_smem_bytes(p.J);
    e = pj_set_lds(pj_fwd_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pj_fwd_kernel, dim3((uint32_t)p.band.B * (uint32_t)p.tiles_per_utt), dim3(kPJThreads), lds, s, p);
    return hipGetLastError();
}

hipError_t launch_pruned_joint_backward(const PrunedJointParams &p, const bool w2max_fresh, hipStream_t s) {
    const PrunedParams &q = p.band;
    hipError_t e = w2max_fresh ? hipSuccess : launch_w2max(p, s);  // (a forward of the same call has just left the entries)
    if (e != hipSuccess) return e;
    const size_t lds = pj_smem_bytes(p.J);
    e = pj_set_lds(pj_bwd_dh_kernel, lds);
    if (e != hipSuccess) return e;
    e = pj_set_lds(pj_bwd_dw_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pj_bwd_dh_kernel, dim3((uint32_t)q.B * (uint32_t)p.tiles_per_utt), dim3(kPJThreads), lds, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const size_t n_enc = (size_t)q.B * (size_t)q.T * (size_t)(p.J / 4);
    hipLaunchKernelGGL(pj_reduce_enc_kernel, dim3((uint32_t)((n_enc + kPJThreads - 1) / kPJThreads)), dim3(kPJThreads), 0, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(pj_reduce_pred_kernel, dim3((uint32_t)q.B * (uint32_t)q.U), dim3(kPJThreads), 0, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(pj_bwd_dw_kernel, dim3((uint32_t)p.vtiles * (uint32_t)p.chunks), dim3(kPJThreads), lds, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const size_t n_w = (size_t)p.J * (size_t)q.V + (size_t)q.V;
    hipLaunchKernelGGL(pj_reduce_w_kernel, dim3((uint32_t)((n_w + kPJThreads - 1) / kPJThreads)), dim3(kPJThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace rnnt
