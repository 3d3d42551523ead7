// rnnt_ctc_kernels.hip -- the CTC loss and the greedy CTC decoder of the auxiliary head (include/rnnt_ctc.h; rnnt_ctc.h for the
// ownership of the states and the workspace).
//
//   ctc_prepare_kernel            per utterance, from the labels alone: the clamped labels, the validity flag (a label equal to the
//                                 blank), and per position the skip bit and the occurrence chain of its symbol (first occurrence?
//                                 next position with the same symbol), which lets the gradient pass sum a repeated symbol's
//                                 occupancies in one thread, in increasing position, without atomics.
//   ctc_rows_kernel<W>            one wavefront per live frame: the log-softmax normaliser (f32, online max / sum, W = 4: 16-byte
//                                 loads, W = 1: rows that are not 16-byte aligned) and the L + 1 edge log-probabilities the sweeps
//                                 need, gathered twice: aligned to the alpha sweep's positions and to the beta sweep's.
//   ctc_sweep_kernel<K, G, WIDE>  ONE launch for both directions: workgroup 2b sweeps alpha, 2b + 1 beta of utterance b.  A thread
//                                 owns K label positions = 2K states; a row depends on the row before it only, so a sweep takes
//                                 T_b steps with every state in flight, and only a position's label state crosses to the
//                                 neighbouring thread (a whole-wave DPP shift, or LDS + one barrier per row in the wide kernel).
//                                 The recurrence is carried in float64 registers, the log(sum of e^-|d|) term on the float32
//                                 units; alpha and beta are stored as float64.  G rows of edge log-probabilities are in flight
//                                 per buffer, two buffers; the stores leave the chain as soon as a row is done.
//   ctc_grad_kernel<W>            one workgroup per frame, one write of EVERY element of grads (zeros for padded frames, which are
//                                 not read): the softmax row staged in LDS in tiles of kCtcGradTile columns, minus the
//                                 per-symbol occupancy sums in the chain's order; the blank's sum is an ordered reduction.
//   ctc_greedy_kernel<W>          one workgroup per utterance: a wavefront per frame takes the argmax (lowest index on ties),
//                                 chunks of kCtcGreedyChunk frames are compacted in order by ballot / popcount and a running offset.
//
// Every sum has an order fixed by V alone in the row pass and by the utterance's own states in the sweeps and the gradient pass: an
// utterance's results do not depend on the batch around it.
#include "rnnt_ctc.h"

#include <limits.h>
#include <math.h>

namespace rnnt {

constexpr float kCtcNegInit = -3.0e38f;  // finite: two lanes without elements merge to (this, 0), not to NaN

struct CtcUtt {
    int Tb, Lb;  // clamped into the tensors
    bool bad;    // out-of-range lengths: the utterance is reported as NaN
};

__device__ __forceinline__ CtcUtt ctc_utt(const CtcParams &p, const int b) {
    const int Tb = p.input_lengths[b], Lb = p.label_lengths[b];
    CtcUtt u;
    u.bad = Tb < 1 || Tb > p.T || Lb < 0 || Lb > p.U - 1;
    u.Tb = min(max(Tb, 1), p.T);
    u.Lb = min(max(Lb, 0), p.U - 1);
    return u;
}

// the W elements of a row that start at element i (W = 1: any alignment; W = 4: V % 4 == 0 and a 16-byte-aligned tensor)
template <int W>
__device__ __forceinline__ void ctc_load(float (&x)[W], const float *row, const int i) {
    if constexpr (W == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(row + i);
        x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
        x[0] = row[i];
    }
}
template <int W>
__device__ __forceinline__ void ctc_store(float *row, const int i, const float (&x)[W]) {
    if constexpr (W == 4)
        *reinterpret_cast<float4 *>(row + i) = make_float4(x[0], x[1], x[2], x[3]);
    else
        row[i] = x[0];
}

// ---------------------------------------------------------------------------------------------
// Prepare.  The labels of one utterance in LDS; thread k looks backwards for an earlier and forwards for the next occurrence of y_k.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) ctc_prepare_kernel(const CtcParams p) {
    __shared__ int s_lab[kMaxU];
    __shared__ int s_bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    const CtcUtt u = ctc_utt(p, b);
    if (tid == 0) s_bad = u.bad ? 1 : 0;
    __syncthreads();
    const int *y = p.labels + (size_t)b * (size_t)(p.U - 1);
    bool blank_seen = false;
    for (int k = tid; k < u.Lb; k += 1024) {
        const int v = min(max(y[k], 0), p.V - 1);
        s_lab[k] = v;
        blank_seen |= v == p.blank;
    }
    if (blank_seen) s_bad = 1;  // (every writer stores the same value)
    __syncthreads();
    int *meta = p.meta + (size_t)b * p.Up, *lab = p.lab + (size_t)b * p.Up;
    for (int k = tid; k < u.Lb; k += 1024) {
        const int v = s_lab[k];
        int m = (k >= 1 && v != s_lab[k - 1]) ? kCtcSkip : 0;
        int j = k - 1;
        while (j >= 0 && s_lab[j] != v) --j;
        if (j < 0) m |= kCtcFirst;
        j = k + 1;
        while (j < u.Lb && s_lab[j] != v) ++j;
        if (j < u.Lb) m |= (j + 1) << kCtcNextShift;
        meta[k] = m;
        lab[k] = v;
    }
    if (tid == 0) p.flags[b] = s_bad;
}

hipError_t launch_ctc_prepare(const CtcParams &p, hipStream_t s) {
    hipLaunchKernelGGL(ctc_prepare_kernel, dim3(p.B), dim3(1024), 0, s, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Row pass.  Lane j takes the pieces j, j + 64, ... (W elements each) of the frame's V logits and keeps a running
// (max, sum of exp(x - max)); the 64 partial pairs are merged by a butterfly that leaves the same bits in every lane.
// ---------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(256) ctc_rows_kernel(const CtcParams p) {
    const int lane = threadIdx.x & 63;
    const uint32_t f = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (f >= (uint32_t)p.B * (uint32_t)p.T) return;
    const int b = (int)(f / (uint32_t)p.T), t = (int)(f - (uint32_t)b * (uint32_t)p.T);
    const CtcUtt u = ctc_utt(p, b);
    if (t >= u.Tb) return;  // padding: not read (the whole wavefront leaves together)

    const int V = p.V;
    const float *row = p.acts + (size_t)f * (size_t)V;
    float mx = kCtcNegInit, s = 0.0f;
#pragma unroll 2
    for (int i = lane * W; i < V; i += 64 * W) {
        float x[W];
        ctc_load<W>(x, row, i);
        float nm = mx;
#pragma unroll
        for (int k = 0; k < W; ++k) nm = fmaxf(nm, x[k]);
        float e = 0.0f;
#pragma unroll
        for (int k = 0; k < W; ++k) e += __expf(x[k] - nm);
        s = s * __expf(mx - nm) + e;
        mx = nm;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float m2 = __shfl_xor(mx, off, 64), s2 = __shfl_xor(s, off, 64);
        const float nm = fmaxf(mx, m2);
        const float a = s * __expf(mx - nm), bsum = s2 * __expf(m2 - nm);
        s = (lane & off) ? bsum + a : a + bsum;  // lower lane's part first on both sides: the pair ends with the same bits
        mx = nm;
    }
    const float lse = mx + __logf(s);
    if (lane == 0) p.lse[f] = lse;
    const float lpb = row[p.blank] - lse;
    const int *lab = p.lab + (size_t)b * p.Up;
    float2 *lpa = p.lpa + (size_t)f * (size_t)p.Up, *lpbeta = p.lpb + (size_t)f * (size_t)p.Up;
    for (int k = lane; k <= u.Lb; k += 64) {
        const float ya = k < u.Lb ? row[lab[k]] - lse : 0.0f;
        const float yb = k >= 1 ? row[lab[k - 1]] - lse : 0.0f;
        lpa[k] = make_float2(lpb, ya);
        lpbeta[k] = make_float2(lpb, yb);
    }
}

hipError_t launch_ctc_rows(const CtcParams &p, hipStream_t s) {
    const bool vec = (p.V % kCtcRowVec == 0) && (((uintptr_t)p.acts & 15) == 0);
    const uint32_t frames = (uint32_t)p.B * (uint32_t)p.T;
    const dim3 grid((frames + 3) / 4);
    if (vec)
        hipLaunchKernelGGL((ctc_rows_kernel<kCtcRowVec>), grid, dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((ctc_rows_kernel<1>), grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Sweeps.  Thread j owns the positions j K ... j K + K - 1 (rnnt_ctc.h).  States outside the lattice are -inf, and their edge
// log-probabilities (never written by the row pass) are never part of a sum.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double ctc_dpp(const double x, const double fill, const bool from_lower) {
    const long long xi = __double_as_longlong(x), fi = __double_as_longlong(fill);
    int lo, hi;
    if (from_lower) {
        lo = __builtin_amdgcn_update_dpp((int)fi, (int)xi, 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
        hi = __builtin_amdgcn_update_dpp((int)(fi >> 32), (int)(xi >> 32), 0x138, 0xf, 0xf, false);
    } else {
        lo = __builtin_amdgcn_update_dpp((int)fi, (int)xi, 0x130 /*wave_shl:1*/, 0xf, 0xf, false);
        hi = __builtin_amdgcn_update_dpp((int)(fi >> 32), (int)(xi >> 32), 0x130, 0xf, 0xf, false);
    }
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// log(e^x + e^y): float64 carry, the term in (0, ln 2] on the float32 units (include/rnnt_ctc.h, Numerics)
__device__ __forceinline__ double ctc_logadd(const double x, const double y) {
    const double hi = fmax(x, y), lo = fmin(x, y);
    const float d = (float)(lo - hi);  // <= 0 (NaN when both are -inf: the result is taken from hi)
    const float term = __logf(1.0f + __expf(d));
    return hi == -INFINITY ? hi : hi + (double)term;
}

// log(e^x + e^y + e^z), the same way: the term in [0, ln 3]
__device__ __forceinline__ double ctc_logadd3(const double x, const double y, const double z) {
    const double m = fmax(fmax(x, y), z);
    const float s = __expf((float)(x - m)) + __expf((float)(y - m)) + __expf((float)(z - m));  // (NaN when all are -inf)
    return m == -INFINITY ? m : m + (double)__logf(s);
}

template <int K>
struct CtcRow {
    float2 e[K];
};

template <int K>
__device__ __forceinline__ void ctc_load_row(CtcRow<K> &d, const float2 *rowp) {
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

template <int K, int G, bool WIDE, bool BETA>
__device__ __forceinline__ void ctc_sweep(const CtcParams &p, double *xch) {
    constexpr int kThreads = WIDE ? kCtcWideThreads : kCtcWaveThreads;
    const int b = blockIdx.x >> 1, tid = threadIdx.x;
    const CtcUtt u = ctc_utt(p, b);
    const int Tb = u.Tb, Lb = u.Lb, Up = p.Up;
    const int u0 = tid * K;
    const float2 *lp = (BETA ? p.lpb : p.lpa) + (size_t)b * p.T * (size_t)Up + u0;
    double2 *out = (BETA ? p.beta : p.alpha) + (size_t)b * p.T * (size_t)Up + u0;

    unsigned skip = 0;  // bit k: the label state of position u0 + k may be entered from the label state two states away
    {
        const int *meta = p.meta + (size_t)b * Up;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (u0 + k < Lb && (meta[u0 + k] & kCtcSkip)) skip |= 1u << k;
    }
    // which states of position u0 + k exist: the blank state for k <= L_b, the label state y_k (alpha) / y_{k-1} (beta)
    auto has_blank = [&](const int k) { return u0 + k <= Lb; };
    auto has_label = [&](const int k) { return BETA ? (u0 + k >= 1 && u0 + k <= Lb) : (u0 + k < Lb); };

    // the virtual row in front of the first: all mass in the blank state the first row is entered through
    double vb[K], vl[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        vb[k] = (u0 + k == (BETA ? Lb : 0)) ? 0.0 : -INFINITY;
        vl[k] = -INFINITY;
    }

    int xs = 0;  // exchanges so far: the wide kernel's buffer parity
    auto neighbour = [&]() {  // the label state of the position below (alpha) / above (beta) this thread's, on the row just done
        double cin;
        if constexpr (WIDE) {
            double *x = xch + (xs & 1) * kThreads;
            x[tid] = BETA ? vl[0] : vl[K - 1];
            __syncthreads();
            if constexpr (BETA)
                cin = tid + 1 < kThreads ? x[tid + 1] : -INFINITY;
            else
                cin = tid ? x[tid - 1] : -INFINITY;
        } else {
            cin = ctc_dpp(BETA ? vl[0] : vl[K - 1], -INFINITY, !BETA);
        }
        ++xs;
        return cin;
    };

    int ls = 0;  // the next step to load: step s reads frame s (alpha) / T_b - 1 - s (beta)
    auto load_block = [&](CtcRow<K>(&buf)[G]) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int s = min(ls, Tb - 1);  // (past the end: a row of this utterance again, not used)
            ctc_load_row<K>(buf[g], lp + (size_t)(BETA ? Tb - 1 - s : s) * Up);
            ++ls;
        }
    };
    auto step = [&](const int s, const CtcRow<K> &d) {
        const int t = BETA ? Tb - 1 - s : s;
        const double cin = neighbour();
        double nb[K], nl[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double from = BETA ? (k + 1 < K ? vl[k + 1 < K ? k + 1 : k] : cin) : (k ? vl[k ? k - 1 : 0] : cin);
            const bool okb = has_blank(k), okl = has_label(k);
            const double eb = (double)(okb ? d.e[k].x : 0.0f), el = (double)(okl ? d.e[k].y : 0.0f);
            const double b2 = ctc_logadd(vb[k], from);
            const double l3 = ctc_logadd3(vl[k], vb[k], ((skip >> k) & 1u) ? from : -INFINITY);
            nb[k] = okb ? eb + b2 : -INFINITY;
            nl[k] = okl ? el + l3 : -INFINITY;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            vb[k] = nb[k], vl[k] = nl[k];
            out[(size_t)t * Up + k] = make_double2(nb[k], nl[k]);
        }
    };

    CtcRow<K> bufA[G], bufB[G];
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

    if constexpr (!BETA) {  // ln P = logaddexp(alpha(T_b - 1, 2 L_b), alpha(T_b - 1, 2 L_b - 1)): -inf when no path exists
        const double cin = neighbour();
        const bool bad = u.bad || p.flags[b] != 0;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (u0 + k == Lb) {
                const double from = k ? vl[k ? k - 1 : 0] : cin;
                const double lnP = bad ? (double)__int_as_float(0x7fc00000) : ctc_logadd(vb[k], from);
                p.lnP[b] = lnP;
                if (p.costs) p.costs[b] = (float)(-lnP);
            }
    }
}

template <int K, int G, bool WIDE>
__global__ void __launch_bounds__(WIDE ? kCtcWideThreads : kCtcWaveThreads) ctc_sweep_kernel(const CtcParams p) {
    __shared__ double xch[WIDE ? 2 * kCtcWideThreads : 2];  // the wide kernel's neighbour exchange, double-buffered by step parity
    if (blockIdx.x & 1)
        ctc_sweep<K, G, WIDE, true>(p, xch);
    else
        ctc_sweep<K, G, WIDE, false>(p, xch);
}

template <int K, int G, bool WIDE>
static hipError_t launch_ctc_sweep_KG(const CtcParams &p, hipStream_t s) {
    hipLaunchKernelGGL((ctc_sweep_kernel<K, G, WIDE>), dim3(2 * p.B), dim3(WIDE ? kCtcWideThreads : kCtcWaveThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_ctc_sweeps(const CtcParams &p, hipStream_t s) {
    // rows in flight per buffer: about 32 floats of registers per thread and buffer
    const CtcTier tier = ctc_tier(p.U);
    if (tier.threads == kCtcWaveThreads) {
        switch (tier.K) {
            case 1: return launch_ctc_sweep_KG<1, 16, false>(p, s);
            case 2: return launch_ctc_sweep_KG<2, 8, false>(p, s);
            case 3: return launch_ctc_sweep_KG<3, 4, false>(p, s);
            case 4: return launch_ctc_sweep_KG<4, 4, false>(p, s);
            case 6: return launch_ctc_sweep_KG<6, 2, false>(p, s);
            case 8: return launch_ctc_sweep_KG<8, 2, false>(p, s);
            case 12: return launch_ctc_sweep_KG<12, 1, false>(p, s);
            case 16: return launch_ctc_sweep_KG<16, 1, false>(p, s);
            default: return hipErrorInvalidValue;
        }
    }
    switch (tier.K) {  // more than 1024 positions: 1024 threads, 128 registers each
        case 2: return launch_ctc_sweep_KG<2, 2, true>(p, s);
        case 3: return launch_ctc_sweep_KG<3, 1, true>(p, s);
        case 4: return launch_ctc_sweep_KG<4, 1, true>(p, s);
        case 6: return launch_ctc_sweep_KG<6, 1, true>(p, s);
        case 8: return launch_ctc_sweep_KG<8, 1, true>(p, s);
        default: return hipErrorInvalidValue;
    }
}

// ---------------------------------------------------------------------------------------------
// Gradient pass.  occ(t, s) = exp(alpha + beta - lp - ln P); the label states' occupancies go to LDS by position, a symbol's first
// occurrence walks its chain through them; the blank states' occupancies are summed per thread in increasing position, then by a
// butterfly of fixed order and the four wavefronts' parts in order.
// ---------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(kCtcGradThreads) ctc_grad_kernel(const CtcParams p, const int tile_cols) {
    extern __shared__ __align__(16) float ctc_smem[];
    float *tile = ctc_smem;                              // [tile_cols] (a multiple of 4)
    float *occ = ctc_smem + tile_cols;                   // [U] the label states' occupancies by position
    int *s_meta = reinterpret_cast<int *>(occ + p.U);    // [U] the chain
    __shared__ float s_part[kCtcGradThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t f = blockIdx.x;
    const int b = (int)(f / (uint32_t)p.T), t = (int)(f - (uint32_t)b * (uint32_t)p.T);
    const CtcUtt u = ctc_utt(p, b);
    const int V = p.V;
    float *grow = p.grads + (size_t)f * (size_t)V;
    const double lnP = p.lnP[b];  // NaN for an invalid utterance
    const bool nan = lnP != lnP;
    if (t >= u.Tb || nan || lnP == -INFINITY) {  // zeros (padding, no path) or NaN (invalid, its clamped frames); the logits are not read
        float z[W];
#pragma unroll
        for (int k = 0; k < W; ++k) z[k] = (t < u.Tb && nan) ? __int_as_float(0x7fc00000) : 0.0f;
        for (int i = tid * W; i < V; i += kCtcGradThreads * W) ctc_store<W>(grow, i, z);
        return;
    }
    const float cs = p.cost_scale ? p.cost_scale[b] : 1.0f;
    const float lse = p.lse[f];
    const size_t base = (size_t)f * (size_t)p.Up;
    const int *meta = p.meta + (size_t)b * p.Up, *lab = p.lab + (size_t)b * p.Up;
    float bsum = 0.0f;
    for (int k = tid; k <= u.Lb; k += kCtcGradThreads) {
        const double2 a = p.alpha[base + k], be = p.beta[base + k];
        const float2 l = p.lpa[base + k];
        bsum += __expf((float)(a.x + be.x - (double)l.x - lnP));
        if (k < u.Lb) {
            const double bl = p.beta[base + k + 1].y;  // beta(t, 2k + 1) is held by position k + 1
            occ[k] = __expf((float)(a.y + bl - (double)l.y - lnP));
            s_meta[k] = meta[k];
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float o = __shfl_xor(bsum, off, 64);
        bsum = (lane & off) ? o + bsum : bsum + o;  // lower lane's part first on both sides
    }
    if (lane == 0) s_part[tid >> 6] = bsum;
    __syncthreads();  // s_part, occ and s_meta are complete
    float btot = s_part[0];
#pragma unroll
    for (int w = 1; w < kCtcGradThreads / 64; ++w) btot += s_part[w];

    const float *row = p.acts + (size_t)f * (size_t)V;
    for (int c0 = 0; c0 < V; c0 += tile_cols) {
        const int n = min(tile_cols, V - c0);
        for (int i = tid * W; i < n; i += kCtcGradThreads * W) {
            float x[W];
            ctc_load<W>(x, row + c0, i);
#pragma unroll
            for (int k = 0; k < W; ++k) tile[i + k] = cs * __expf(x[k] - lse);
        }
        __syncthreads();
        for (int k = tid; k < u.Lb; k += kCtcGradThreads) {
            const int m = s_meta[k];
            if (!(m & kCtcFirst)) continue;
            const int v = lab[k] - c0;
            if (v < 0 || v >= n) continue;
            float sum = occ[k];
            for (int nx = m >> kCtcNextShift; nx; nx = s_meta[nx - 1] >> kCtcNextShift) sum += occ[nx - 1];
            tile[v] -= cs * sum;  // the symbol's one writer (no label equals the blank: that utterance is invalid)
        }
        if (tid == 0 && p.blank >= c0 && p.blank < c0 + n) tile[p.blank - c0] -= cs * btot;
        __syncthreads();
        for (int i = tid * W; i < n; i += kCtcGradThreads * W) {
            float x[W];
#pragma unroll
            for (int k = 0; k < W; ++k) x[k] = tile[i + k];
            ctc_store<W>(grow + c0, i, x);
        }
        __syncthreads();
    }
}

hipError_t launch_ctc_grad(const CtcParams &p, hipStream_t s) {
    const bool vec = (p.V % 4 == 0) && ((((uintptr_t)p.acts | (uintptr_t)p.grads) & 15) == 0);
    const int tile_cols = min(kCtcGradTile, (p.V + 3) / 4 * 4);
    const size_t lds = ((size_t)tile_cols + 2 * (size_t)p.U) * sizeof(float);
    const dim3 grid((uint32_t)p.B * (uint32_t)p.T);
    hipError_t e;
    if (vec) {
        if ((e = set_lds(ctc_grad_kernel<4>, lds)) != hipSuccess) return e;
        hipLaunchKernelGGL((ctc_grad_kernel<4>), grid, dim3(kCtcGradThreads), lds, s, p, tile_cols);
    } else {
        if ((e = set_lds(ctc_grad_kernel<1>, lds)) != hipSuccess) return e;
        hipLaunchKernelGGL((ctc_grad_kernel<1>), grid, dim3(kCtcGradThreads), lds, s, p, tile_cols);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Greedy.  s_a[i + 1] = the argmax of frame c0 + i of the chunk, s_a[0] = the argmax of the frame in front of the chunk (the blank
// in front of frame 0: a_0 is emitted iff it is no blank).  Every wavefront takes the same ballot, so all of them carry the count.
// ---------------------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(256) ctc_greedy_kernel(const CtcGreedyParams p) {
    __shared__ int s_a[kCtcGreedyChunk + 1];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Tb = min(max(p.input_lengths[b], 0), p.T);
    const int V = p.V;
    int *tok = p.tokens + (size_t)b * (size_t)p.T;
    int *frm = p.token_frames ? p.token_frames + (size_t)b * (size_t)p.T : nullptr;
    int count = 0;
    if (tid == 0) s_a[0] = p.blank;
    for (int c0 = 0; c0 < Tb; c0 += kCtcGreedyChunk) {
        __syncthreads();  // s_a[0] is set and the chunk before is read
        for (int i = wave; i < kCtcGreedyChunk && c0 + i < Tb; i += 4) {
            const float *row = p.acts + ((size_t)b * (size_t)p.T + (size_t)(c0 + i)) * (size_t)V;
            float bv = -INFINITY;
            int bi = INT_MAX;
            for (int j = lane * W; j < V; j += 64 * W) {
                float x[W];
                ctc_load<W>(x, row, j);
#pragma unroll
                for (int k = 0; k < W; ++k)
                    if (x[k] > bv || (x[k] == bv && j + k < bi)) bv = x[k], bi = j + k;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float ov = __shfl_xor(bv, off, 64);
                const int oi = __shfl_xor(bi, off, 64);
                if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
            }
            if (lane == 0) s_a[i + 1] = bi == INT_MAX ? 0 : bi;  // (a row of NaN alone)
        }
        __syncthreads();
        const int t = c0 + lane;
        const int a = t < Tb ? s_a[lane + 1] : p.blank, prev = s_a[lane];
        const bool emit = t < Tb && a != p.blank && a != prev;
        const unsigned long long mask = __ballot(emit);
        if (wave == 0 && emit) {
            const int pos = count + __popcll(mask & ((1ull << lane) - 1ull));  // pos <= t < maxT
            tok[pos] = a;
            if (frm) frm[pos] = t;
        }
        count += __popcll(mask);
        const int last = s_a[kCtcGreedyChunk];  // (of a full chunk: a partial one is the last)
        __syncthreads();
        if (tid == 0) s_a[0] = last;
    }
    for (int i = count + tid; i < p.T; i += 256) {
        tok[i] = -1;
        if (frm) frm[i] = -1;
    }
    if (tid == 0) p.lengths[b] = count;
}

hipError_t launch_ctc_greedy(const CtcGreedyParams &p, hipStream_t s) {
    const bool vec = (p.V % 4 == 0) && (((uintptr_t)p.acts & 15) == 0);
    if (vec)
        hipLaunchKernelGGL((ctc_greedy_kernel<4>), dim3(p.B), dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((ctc_greedy_kernel<1>), dim3(p.B), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace rnnt
