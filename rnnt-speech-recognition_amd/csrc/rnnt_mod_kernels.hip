// rnnt_mod_kernels.hip -- the transducer loss on the MODIFIED lattice: every frame emits exactly one of {blank, next label}
// (include/rnnt_modified.h; rnnt_mod.h for the recurrence and the workspace).
//
//   mod_cells_kernel<L, W>        one read of the logits: log-softmax normaliser per live in-band cell (f32, online max / sum,
//                                 L lanes per cell, W = 4: 16-byte loads, W = 1: rows that are not 16-byte aligned), stored as
//                                 {lpb, lpl} and lse.  HBM-bound.
//   mod_sweep_kernel<K, G, WIDE>  ONE launch for both directions: workgroup 2b sweeps alpha, 2b + 1 beta of utterance b.  Lanes map
//                                 to lattice columns (K per thread); a row depends on the row before it only, so the sweep takes
//                                 T_b steps with every column in flight.  The recurrence is carried in float64 registers, the
//                                 log(1 + e^-|d|) term of a log-add on the float32 units; alpha and beta are stored as float64.
//                                 One wavefront up to 1024 columns (the neighbour's column by DPP), 1024 threads beyond (through
//                                 LDS, one barrier per row).
//   mod_grad_kernel<L, W>         one read of the logits, one write of EVERY element of grads: zeros for padded cells and for live
//                                 cells outside the band (neither is read).  HBM-bound.
//
// Every sum has an order fixed by V alone in the cell pass and by the utterance's own cells in the sweeps: an utterance's results
// do not depend on the batch around it.
#include "rnnt_mod.h"

#include <math.h>

namespace rnnt {

constexpr float kModNegInit = -3.0e38f;  // finite: two lanes without elements merge to (this, 0), not to NaN

struct ModCell {
    int b, t, u;
    int Tb, Ub;  // clamped into the tensor
    bool bad;    // out-of-range lengths: the utterance is reported as NaN
    bool live;   // t < T_b, u <= L_b
    bool band;   // live and reachable: u <= t, L_b - u <= T_b - t
};

__device__ __forceinline__ ModCell mod_cell(const ModParams &p, const uint32_t c) {
    ModCell m;
    const uint32_t bt = fdiv(c, p.divU);
    m.u = (int)(c - bt * (uint32_t)p.U);
    m.b = (int)fdiv(bt, p.divT);
    m.t = (int)(bt - (uint32_t)m.b * (uint32_t)p.T);
    const int Tb = p.input_lengths[m.b], Ub = p.label_lengths[m.b];
    m.bad = Tb < 1 || Tb > p.T || Ub < 0 || Ub > p.U - 1;
    m.Tb = min(max(Tb, 1), p.T);
    m.Ub = min(max(Ub, 0), p.U - 1);
    m.live = m.t < m.Tb && m.u <= m.Ub;
    m.band = m.live && m.u <= m.t && m.Ub - m.u <= m.Tb - m.t;
    return m;
}

// the W elements of a row that start at element i (W = 1: any alignment; W = 4: V % 4 == 0 and a 16-byte-aligned tensor)
template <int W>
__device__ __forceinline__ void mod_load(float (&x)[W], const float *row, const int i) {
    if constexpr (W == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(row + i);
        x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
        x[0] = row[i];
    }
}
template <int W>
__device__ __forceinline__ void mod_store(float *row, const int i, const float (&x)[W]) {
    if constexpr (W == 4)
        *reinterpret_cast<float4 *>(row + i) = make_float4(x[0], x[1], x[2], x[3]);
    else
        row[i] = x[0];
}

// ---------------------------------------------------------------------------------------------
// Cell pass.  A group of L lanes owns one lattice cell; lane j takes the pieces j, j + L, ... (W elements each) of its V logits and
// keeps a running (max, sum of exp(x - max)); the L partial pairs are merged by a butterfly.
// ---------------------------------------------------------------------------------------------
template <int L, int W>
__global__ void __launch_bounds__(256) mod_cells_kernel(const ModParams p) {
    constexpr int kCellsPerBlock = 256 / L;
    const int tid = threadIdx.x;
    const int j = tid % L;
    const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.T * (uint32_t)p.U;
    const uint32_t c = blockIdx.x * (uint32_t)kCellsPerBlock + (uint32_t)(tid / L);
    if (c >= ncells) return;
    const ModCell m = mod_cell(p, c);
    if (!m.band) return;  // padding, or no path passes here: not read (the whole group leaves together)

    const int V = p.V;
    const float *row = p.acts + (size_t)c * (size_t)V;
    float mx = kModNegInit, s = 0.0f;
#pragma unroll 2
    for (int i = j * W; i < V; i += L * W) {
        float x[W];
        mod_load<W>(x, row, i);
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
    for (int off = L / 2; off >= 1; off >>= 1) {
        const float m2 = __shfl_xor(mx, off, 64), s2 = __shfl_xor(s, off, 64);
        const float nm = fmaxf(mx, m2);
        const float a = s * __expf(mx - nm), bsum = s2 * __expf(m2 - nm);
        s = (j & off) ? bsum + a : a + bsum;  // lower lane's part first on both sides: the pair ends with the same bits
        mx = nm;
    }
    if (j != 0) return;
    const float lse = mx + __logf(s);
    float2 out;
    out.x = row[p.blank] - lse;
    out.y = 0.0f;
    if (m.u < m.Ub) {
        int lab = p.labels[(size_t)m.b * (size_t)(p.U - 1) + m.u];
        lab = min(max(lab, 0), V - 1);
        out.y = row[lab] - lse;
    }
    p.lp[((size_t)m.b * p.T + m.t) * (size_t)p.Up + m.u] = out;
    p.lse[c] = lse;
}

// ---------------------------------------------------------------------------------------------
// Gradient pass: the same lane map.  With e_b = exp(alpha + lpb + beta(t+1,u) - ln P), e_l = exp(alpha + lpl + beta(t+1,u+1) - ln P):
//   grads[v] = cost_scale ((e_b + e_l + lambda e_l) softmax[v] - [v == blank] e_b - [v == y_u] (1 + lambda) e_l)
// ---------------------------------------------------------------------------------------------
template <int L, int W>
__global__ void __launch_bounds__(256) mod_grad_kernel(const ModParams p) {
    constexpr int kCellsPerBlock = 256 / L;
    const int tid = threadIdx.x;
    const int j = tid % L;
    const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.T * (uint32_t)p.U;
    const uint32_t c = blockIdx.x * (uint32_t)kCellsPerBlock + (uint32_t)(tid / L);
    if (c >= ncells) return;
    const ModCell m = mod_cell(p, c);
    const int V = p.V;
    float *grow = p.grads + (size_t)c * (size_t)V;
    const double lnP = p.lnP[m.b];  // NaN for out-of-range lengths
    if (!m.live || (!m.bad && (!m.band || lnP == -INFINITY))) {  // exact zeros; the logits are not read
        float z[W];
#pragma unroll
        for (int k = 0; k < W; ++k) z[k] = 0.0f;
        for (int i = j * W; i < V; i += L * W) mod_store<W>(grow, i, z);
        return;
    }
    if (m.bad) {
        float z[W];
#pragma unroll
        for (int k = 0; k < W; ++k) z[k] = __int_as_float(0x7fc00000);
        for (int i = j * W; i < V; i += L * W) mod_store<W>(grow, i, z);
        return;
    }
    const size_t cu = ((size_t)m.b * p.T + m.t) * (size_t)p.Up + m.u;
    const size_t nu = ((size_t)m.b * (p.T + 1) + m.t + 1) * (size_t)p.Up + m.u;
    const double a = p.alpha[cu];
    const float2 lp = p.lp[cu];
    const float eb = __expf((float)(a + (double)lp.x + p.beta[nu] - lnP));
    float el = 0.0f;
    int lab = -1;
    if (m.u < m.Ub) {
        el = __expf((float)(a + (double)lp.y + p.beta[nu + 1] - lnP));
        lab = p.labels[(size_t)m.b * (size_t)(p.U - 1) + m.u];
        lab = min(max(lab, 0), V - 1);
    }
    const float cs = p.cost_scale ? p.cost_scale[m.b] : 1.0f;
    const float coef = cs * (eb + el + p.fe_lambda * el);
    const float sb = cs * eb, sl = cs * ((1.0f + p.fe_lambda) * el);
    const float lse = p.lse[c];
    const float *row = p.acts + (size_t)c * (size_t)V;
#pragma unroll 2
    for (int i = j * W; i < V; i += L * W) {
        float x[W];
        mod_load<W>(x, row, i);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            float g = coef * __expf(x[k] - lse);
            g -= (i + k == p.blank) ? sb : 0.0f;
            g -= (i + k == lab) ? sl : 0.0f;
            x[k] = g;
        }
        mod_store<W>(grow, i, x);
    }
}

// lanes per cell: the smallest power of two that gives every piece of a row a lane, at most one wavefront
template <int W, typename F>
static hipError_t mod_dispatch_L(const int V, F &&f) {
    using std::integral_constant;
    const int pieces = (V + W - 1) / W;
    if (pieces <= 1) return f(integral_constant<int, 1>());
    if (pieces <= 2) return f(integral_constant<int, 2>());
    if (pieces <= 4) return f(integral_constant<int, 4>());
    if (pieces <= 8) return f(integral_constant<int, 8>());
    if (pieces <= 16) return f(integral_constant<int, 16>());
    if (pieces <= 32) return f(integral_constant<int, 32>());
    return f(integral_constant<int, 64>());
}

template <bool GRAD, int W>
static hipError_t launch_mod_percell(const ModParams &p, hipStream_t s) {
    return mod_dispatch_L<W>(p.V, [&](auto l) {
        constexpr int L = decltype(l)::value;
        const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.T * (uint32_t)p.U;
        const uint32_t per = 256 / L;
        const uint32_t grid = (ncells + per - 1) / per;
        if (GRAD)
            hipLaunchKernelGGL((mod_grad_kernel<L, W>), dim3(grid), dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((mod_cells_kernel<L, W>), dim3(grid), dim3(256), 0, s, p);
        return hipGetLastError();
    });
}

hipError_t launch_mod_cells(const ModParams &p, hipStream_t s) {
    const bool vec = (p.V % 4 == 0) && (((uintptr_t)p.acts & 15) == 0);
    return vec ? launch_mod_percell<false, 4>(p, s) : launch_mod_percell<false, 1>(p, s);
}

hipError_t launch_mod_grad(const ModParams &p, hipStream_t s) {
    const bool vec = (p.V % 4 == 0) && ((((uintptr_t)p.acts | (uintptr_t)p.grads) & 15) == 0);
    return vec ? launch_mod_percell<true, 4>(p, s) : launch_mod_percell<true, 1>(p, s);
}

// ---------------------------------------------------------------------------------------------
// Sweeps.  Thread j owns the lattice columns j K ... j K + K - 1; only the edge column's value crosses to the neighbouring thread
// (a whole-wave DPP shift, or LDS + one barrier per row in the wide kernel).  Cells outside the band are -inf and their {lpb, lpl}
// (never written by the cell pass) are never part of a sum.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double mod_dpp(const double x, const double fill, const bool from_lower) {
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

// log(e^x + e^y): float64 carry, the term in (0, ln 2] on the float32 units (include/rnnt.h, Numerics)
__device__ __forceinline__ double mod_logadd(const double x, const double y) {
    const double hi = fmax(x, y), lo = fmin(x, y);
    const float d = (float)(lo - hi);  // <= 0 (NaN when both are -inf: the result is taken from hi)
    const float term = __logf(1.0f + __expf(d));
    return hi == -INFINITY ? hi : hi + (double)term;
}

template <int K>
struct ModRow {
    float2 e[K];
};

template <int K>
__device__ __forceinline__ void mod_load_row(ModRow<K> &d, const float2 *rowp) {
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

template <int K>
__device__ __forceinline__ void mod_store_row(double *rowp, const double (&v)[K]) {
    if constexpr (K % 2 == 0) {
        double2 *q = reinterpret_cast<double2 *>(rowp);
#pragma unroll
        for (int k = 0; k < K / 2; ++k) q[k] = make_double2(v[2 * k], v[2 * k + 1]);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) rowp[k] = v[k];
    }
}

template <int K, int G, bool WIDE, bool BETA>
__device__ __forceinline__ void mod_sweep(const ModParams &p, double *xch) {
    constexpr int kThreads = WIDE ? 1024 : 64;
    const int b = blockIdx.x >> 1, tid = threadIdx.x;
    int Tb = p.input_lengths[b], Ub = p.label_lengths[b];
    const bool bad = Tb < 1 || Tb > p.T || Ub < 0 || Ub > p.U - 1;
    Tb = min(max(Tb, 1), p.T);
    Ub = min(max(Ub, 0), p.U - 1);
    const int Up = p.Up;
    const int u0 = tid * K;
    const float2 *lp = p.lp + (size_t)b * p.T * (size_t)Up + u0;
    double *out = (BETA ? p.beta + (size_t)b * (p.T + 1) * (size_t)Up : p.alpha + (size_t)b * p.T * (size_t)Up) + u0;
    auto in_band = [&](const int t, const int u) { return u <= t && u <= Ub && Ub - u <= Tb - t; };

    double v[K];  // alpha(0, .) / beta(T_b, .)
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (u0 + k == (BETA ? Ub : 0)) ? 0.0 : -INFINITY;
    if (BETA) mod_store_row<K>(out + (size_t)Tb * Up, v);

    int ls = 0;  // the next step to load: step s reads lattice row s (alpha) / T_b - 1 - s (beta)
    auto load_block = [&](ModRow<K>(&buf)[G]) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int s = min(ls, Tb - 1);  // (past the end: a row of this utterance again, not used)
            mod_load_row<K>(buf[g], lp + (size_t)(BETA ? Tb - 1 - s : s) * Up);
            ++ls;
        }
    };
    auto step = [&](const int s, const ModRow<K> &d) {
        const int t = BETA ? Tb - 1 - s : s;  // the row of the edges: (t, u) -> (t + 1, u) and (t + 1, u + 1)
        double stay[K], move[K];
        if constexpr (!BETA) {
            mod_store_row<K>(out + (size_t)t * Up, v);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int u = u0 + k;
                const bool ok = in_band(t, u);
                stay[k] = v[k] + (double)(ok ? d.e[k].x : 0.0f);
                move[k] = v[k] + (double)((ok && u < Ub) ? d.e[k].y : 0.0f);
            }
            double cin;
            if constexpr (WIDE) {
                double *x = xch + (s & 1) * kThreads;
                x[tid] = move[K - 1];
                __syncthreads();
                cin = tid ? x[tid - 1] : -INFINITY;
            } else {
                cin = mod_dpp(move[K - 1], -INFINITY, true);
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double from = k ? move[k - 1] : cin;
                v[k] = in_band(t + 1, u0 + k) ? mod_logadd(stay[k], from) : -INFINITY;  // (row T_b: column L_b alone)
            }
        } else {
            double cin;
            if constexpr (WIDE) {
                double *x = xch + (s & 1) * kThreads;
                x[tid] = v[0];
                __syncthreads();
                cin = tid + 1 < kThreads ? x[tid + 1] : -INFINITY;
            } else {
                cin = mod_dpp(v[0], -INFINITY, false);
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int u = u0 + k;
                const bool ok = in_band(t, u);
                stay[k] = v[k] + (double)(ok ? d.e[k].x : 0.0f);
                move[k] = (k + 1 < K ? v[k + 1] : cin) + (double)((ok && u < Ub) ? d.e[k].y : 0.0f);
            }
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = in_band(t, u0 + k) ? mod_logadd(stay[k], move[k]) : -INFINITY;
            mod_store_row<K>(out + (size_t)t * Up, v);
        }
    };

    ModRow<K> bufA[G], bufB[G];
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

    if constexpr (!BETA) {  // ln P = alpha(T_b, L_b): -inf when no path exists (L_b > T_b)
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (u0 + k == Ub) {
                const double lnP = bad ? (double)__int_as_float(0x7fc00000) : v[k];
                p.lnP[b] = lnP;
                if (p.costs) p.costs[b] = (float)(-lnP);
            }
    }
}

template <int K, int G, bool WIDE>
__global__ void __launch_bounds__(WIDE ? 1024 : 64) mod_sweep_kernel(const ModParams p) {
    __shared__ double xch[WIDE ? 2 * 1024 : 2];  // the wide kernel's neighbour exchange, double-buffered by step parity
    if (blockIdx.x & 1)
        mod_sweep<K, G, WIDE, true>(p, xch);
    else
        mod_sweep<K, G, WIDE, false>(p, xch);
}

template <int K, int G, bool WIDE>
static hipError_t launch_sweep_KG(const ModParams &p, hipStream_t s) {
    hipLaunchKernelGGL((mod_sweep_kernel<K, G, WIDE>), dim3(2 * p.B), dim3(WIDE ? 1024 : 64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_mod_sweeps(const ModParams &p, hipStream_t s) {
    // rows in flight per buffer: about 32 cells of registers per thread and buffer
    switch (sweep_K(p.U)) {
        case 1: return launch_sweep_KG<1, 16, false>(p, s);
        case 2: return launch_sweep_KG<2, 16, false>(p, s);
        case 3: return launch_sweep_KG<3, 8, false>(p, s);
        case 4: return launch_sweep_KG<4, 8, false>(p, s);
        case 6: return launch_sweep_KG<6, 4, false>(p, s);
        case 8: return launch_sweep_KG<8, 4, false>(p, s);
        case 12: return launch_sweep_KG<12, 2, false>(p, s);
        case 16: return launch_sweep_KG<16, 2, false>(p, s);
        default: break;
    }
    switch (align_wide_K(p.U)) {  // more than 1024 columns: 1024 threads, 128 registers each
        case 2: return launch_sweep_KG<2, 2, true>(p, s);
        case 3: return launch_sweep_KG<3, 2, true>(p, s);
        case 4: return launch_sweep_KG<4, 1, true>(p, s);
        case 6: return launch_sweep_KG<6, 1, true>(p, s);
        case 8: return launch_sweep_KG<8, 1, true>(p, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace rnnt
