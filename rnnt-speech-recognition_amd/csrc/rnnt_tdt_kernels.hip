// rnnt_tdt_kernels.hip -- the token-and-duration (TDT) transducer loss on materialised logits (include/rnnt_tdt.h; rnnt_tdt.h for the
// lattice and the workspace).
//
//   tdt_cells_kernel<L, W>   one streaming read of the logits (the cell's blank, label and D duration logits are then read again for
//                            the weights: cache hits): per live cell the two log-softmax normalisers (tokens [0, V), durations
//                            [V, V + D); f32, online max / sum, L lanes per cell, W = 4: 16-byte loads, W = 1: rows that are not
//                            16-byte aligned), stored as the 2 D edge weights wb_i, wl_i (sigma folded in) and {lseV, lseD}.
//   tdt_sweep_kernel         ONE launch for both directions: workgroup 2b sweeps alpha, 2b + 1 beta of utterance b.  Lanes are
//                            lattice columns, one per thread; a step is one skewed row n = t + u.  A row depends on the dmax + 1
//                            rows before (alpha) / after (beta) it: they are kept in an LDS ring of kTdtRing rows, one barrier
//                            per step.  The weights of the next step are loaded while this one computes.  The recurrence is carried
//                            in float64, the log of the sum of exponentials on the float32 units; alpha and beta are stored as
//                            float64.
//   tdt_grad_kernel<L, W>    one read of the logits of the cells that carry mass, one write of EVERY element of grads: zeros for padded cells and for cells no
//                            path crosses (neither is read).
//
// Every sum has an order fixed by V, D and the utterance's own cells: an utterance's results do not depend on the batch around it.
#include "rnnt_tdt.h"

#include <math.h>

namespace rnnt {

constexpr float kTdtNegInit = -3.0e38f;         // finite: two lanes without elements merge to (this, 0), not to NaN
constexpr int kTdtRing = kTdtMaxDuration + 2;  // rows n - dmax - 1 ... n

struct TdtCell {
    int b, t, u;
    int Tb, Ub;  // clamped into the tensor
    bool bad;    // out-of-range lengths: the utterance is reported as NaN
    bool live;   // t < T_b, u <= L_b
};

__device__ __forceinline__ TdtCell tdt_cell(const TdtParams &p, const uint32_t c) {
    TdtCell m;
    const uint32_t bt = fdiv(c, p.divU);
    m.u = (int)(c - bt * (uint32_t)p.U);
    m.b = (int)fdiv(bt, p.divT);
    m.t = (int)(bt - (uint32_t)m.b * (uint32_t)p.T);
    const int Tb = p.input_lengths[m.b], Ub = p.label_lengths[m.b];
    m.bad = Tb < 1 || Tb > p.T || Ub < 0 || Ub > p.U - 1;
    m.Tb = min(max(Tb, 1), p.T);
    m.Ub = min(max(Ub, 0), p.U - 1);
    m.live = m.t < m.Tb && m.u <= m.Ub;
    return m;
}

// the W elements of a row that start at element i (W = 1: any alignment; W = 4: (V + D) % 4 == 0 and a 16-byte-aligned tensor)
template <int W>
__device__ __forceinline__ void tdt_load(float (&x)[W], const float *row, const int i) {
    if constexpr (W == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(row + i);
        x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
        x[0] = row[i];
    }
}
template <int W>
__device__ __forceinline__ void tdt_store(float *row, const int i, const float (&x)[W]) {
    if constexpr (W == 4)
        *reinterpret_cast<float4 *>(row + i) = make_float4(x[0], x[1], x[2], x[3]);
    else
        row[i] = x[0];
}

// the merge of two (max, sum) pairs across lanes `off` apart; the lower lane's part first on both sides: the same bits in both
__device__ __forceinline__ void tdt_merge(float &mx, float &s, const int j, const int off) {
    const float m2 = __shfl_xor(mx, off, 64), s2 = __shfl_xor(s, off, 64);
    const float nm = fmaxf(mx, m2);
    const float a = s * __expf(mx - nm), bsum = s2 * __expf(m2 - nm);
    s = (j & off) ? bsum + a : a + bsum;
    mx = nm;
}

// ---------------------------------------------------------------------------------------------
// Cell pass.  A group of L lanes owns one lattice cell; lane j takes the pieces j, j + L, ... (W elements each) of its V + D logits
// and keeps a running (max, sum of exp(x - max)) for the tokens and one for the durations; the partial pairs are merged by butterflies.
// ---------------------------------------------------------------------------------------------
template <int L, int W>
__global__ void __launch_bounds__(256) tdt_cells_kernel(const TdtParams p) {
    constexpr int kCellsPerBlock = 256 / L;
    const int tid = threadIdx.x;
    const int j = tid % L;
    const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.T * (uint32_t)p.U;
    const uint32_t c = blockIdx.x * (uint32_t)kCellsPerBlock + (uint32_t)(tid / L);
    if (c >= ncells) return;
    const TdtCell m = tdt_cell(p, c);
    if (!m.live) return;  // padding: not read (the whole group leaves together)

    const int V = p.V, D = p.D, R = V + D;
    const float *row = p.acts + (size_t)c * (size_t)R;
    float mv = kTdtNegInit, sv = 0.0f, md = kTdtNegInit, sd = 0.0f;
#pragma unroll 2
    for (int i = j * W; i < R; i += L * W) {
        float x[W];
        tdt_load<W>(x, row, i);
        float nv = mv, nd = md;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const bool tok = i + k < V;
            nv = tok ? fmaxf(nv, x[k]) : nv;
            nd = tok ? nd : fmaxf(nd, x[k]);
        }
        float ev = 0.0f, ed = 0.0f;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const bool tok = i + k < V;
            const float e = __expf(x[k] - (tok ? nv : nd));
            ev += tok ? e : 0.0f;
            ed += tok ? 0.0f : e;
        }
        sv = sv * __expf(mv - nv) + ev;
        sd = sd * __expf(md - nd) + ed;
        mv = nv, md = nd;
    }
#pragma unroll
    for (int off = L / 2; off >= 1; off >>= 1) {
        tdt_merge(mv, sv, j, off);
        tdt_merge(md, sd, j, off);
    }
    const float lseV = mv + __logf(sv), lseD = md + __logf(sd);
    // the 2 + D logits the weights need are read again here (the lines are in cache) rather than kept from the streaming pass: which
    // lane holds them depends on V, the blank and the label
    const float lpb = (row[p.blank] - lseV) - p.sigma;
    float lpl = 0.0f;
    if (m.u < m.Ub) {
        int lab = p.labels[(size_t)m.b * (size_t)(p.U - 1) + m.u];
        lab = min(max(lab, 0), V - 1);
        lpl = (row[lab] - lseV) - p.sigma;
    }
    const size_t plane = (size_t)p.N * (size_t)p.Up;
    float *w = p.w + (size_t)m.b * (size_t)(2 * D) * plane + (size_t)(m.t + m.u) * (size_t)p.Up + m.u;
    for (int i = j; i < D; i += L) {
        const float ld = row[V + i] - lseD;
        w[(size_t)i * plane] = lpb + ld;
        w[(size_t)(D + i) * plane] = lpl + ld;
    }
    if (j == 0) p.lse[c] = make_float2(lseV, lseD);
}

// ---------------------------------------------------------------------------------------------
// Gradient pass: the same lane map.  Edge 2 i is the blank edge, 2 i + 1 the label edge of duration i; its mass
//   e = exp(alpha(t,u) + w + beta(target) - ln P), 0 for an edge that does not exist,
// is computed once per cell (lane k % L takes edge k) and shared through LDS.  g_b / g_l = the sums over the blank / label edges in
// the order of i, g_i = e(2 i) + e(2 i + 1), m = g_b + g_l:
//   grads[v]     = cost_scale (m softmax_tokens[v] - [v == blank] g_b - [v == y_u] g_l)
//   grads[V + i] = cost_scale (m softmax_durations[i] - g_i)
// ---------------------------------------------------------------------------------------------
template <int L, int W>
__global__ void __launch_bounds__(256) tdt_grad_kernel(const TdtParams p) {
    constexpr int kCellsPerBlock = 256 / L;
    __shared__ float esh[kCellsPerBlock][2 * kTdtMaxD];
    const int tid = threadIdx.x;
    const int j = tid % L, ci = tid / L;
    const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.T * (uint32_t)p.U;
    const uint32_t c = blockIdx.x * (uint32_t)kCellsPerBlock + (uint32_t)ci;
    const bool inside = c < ncells;
    const TdtCell m = tdt_cell(p, inside ? c : 0u);
    const int V = p.V, D = p.D, R = V + D;
    const double lnP = p.lnP[m.b];  // NaN for out-of-range lengths
    const bool mass = inside && m.live && !m.bad && lnP != -INFINITY;
    if (mass) {
        const int n = m.t + m.u;
        const size_t plane = (size_t)p.N * (size_t)p.Up;
        const size_t node = (size_t)m.b * plane + (size_t)n * (size_t)p.Up + m.u;
        const double a = p.alpha[node] - lnP;
        const float *w = p.w + (size_t)m.b * (size_t)(2 * D) * plane + (size_t)n * (size_t)p.Up + m.u;
#pragma unroll
        for (int k = 0; k < 2 * kTdtMaxD; ++k) {
            if (k < 2 * D && (k & (L - 1)) == j) {
                const int i = k >> 1, d = p.dur[k >> 1];
                const bool label = k & 1;
                const bool exists = label ? (m.u < m.Ub && m.t + d < m.Tb)
                                          : (d > 0 && (m.t + d < m.Tb || (m.t + d == m.Tb && m.u == m.Ub)));
                float e = 0.0f;
                if (exists && a != -INFINITY) {
                    const double bt = p.beta[node + (size_t)(label ? d + 1 : d) * (size_t)p.Up + (label ? 1 : 0)];
                    const float wt = w[(size_t)(label ? D + i : i) * plane];
                    e = __expf((float)(a + (double)wt + bt));  // (beta = -inf: 0)
                }
                esh[ci][k] = e;
            }
        }
    }
    __syncthreads();
    if (!inside) return;
    float *grow = p.grads + (size_t)c * (size_t)R;
    float gb = 0.0f, gl = 0.0f;
    if (mass) {
#pragma unroll
        for (int i = 0; i < kTdtMaxD; ++i)
            if (i < D) gb += esh[ci][2 * i], gl += esh[ci][2 * i + 1];
    }
    const float tot = gb + gl;
    if (!m.live || (!m.bad && !(tot > 0.0f))) {  // padding, or no path crosses the cell: exact zeros; the logits are not read
        float z[W];
#pragma unroll
        for (int k = 0; k < W; ++k) z[k] = 0.0f;
        for (int i = j * W; i < R; i += L * W) tdt_store<W>(grow, i, z);
        return;
    }
    if (m.bad) {
        float z[W];
#pragma unroll
        for (int k = 0; k < W; ++k) z[k] = __int_as_float(0x7fc00000);
        for (int i = j * W; i < R; i += L * W) tdt_store<W>(grow, i, z);
        return;
    }
    int lab = -1;
    if (m.u < m.Ub) {
        lab = p.labels[(size_t)m.b * (size_t)(p.U - 1) + m.u];
        lab = min(max(lab, 0), V - 1);
    }
    const float cs = p.cost_scale ? p.cost_scale[m.b] : 1.0f;
    const float coef = cs * tot, sb = cs * gb, sl = cs * gl;
    const float2 lse = p.lse[c];
    const float *row = p.acts + (size_t)c * (size_t)R;
#pragma unroll 2
    for (int i = j * W; i < R; i += L * W) {
        float x[W];
        tdt_load<W>(x, row, i);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const int v = i + k;
            float g;
            if (v < V) {
                g = coef * __expf(x[k] - lse.x);
                g -= (v == p.blank) ? sb : 0.0f;
                g -= (v == lab) ? sl : 0.0f;
            } else {
                const int di = v - V;
                g = coef * __expf(x[k] - lse.y) - cs * (esh[ci][2 * di] + esh[ci][2 * di + 1]);
            }
            x[k] = g;
        }
        tdt_store<W>(grow, i, x);
    }
}

// lanes per cell: the smallest power of two that gives every piece of a row a lane, at most one wavefront
template <int W, typename F>
static hipError_t tdt_dispatch_L(const int R, F &&f) {
    using std::integral_constant;
    const int pieces = (R + W - 1) / W;
    if (pieces <= 1) return f(integral_constant<int, 1>());
    if (pieces <= 2) return f(integral_constant<int, 2>());
    if (pieces <= 4) return f(integral_constant<int, 4>());
    if (pieces <= 8) return f(integral_constant<int, 8>());
    if (pieces <= 16) return f(integral_constant<int, 16>());
    if (pieces <= 32) return f(integral_constant<int, 32>());
    return f(integral_constant<int, 64>());
}

template <bool GRAD, int W>
static hipError_t launch_tdt_percell(const TdtParams &p, hipStream_t s) {
    return tdt_dispatch_L<W>(p.V + p.D, [&](auto l) {
        constexpr int L = decltype(l)::value;
        const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.T * (uint32_t)p.U;
        const uint32_t per = 256 / L;
        const uint32_t grid = (ncells + per - 1) / per;
        if (GRAD)
            hipLaunchKernelGGL((tdt_grad_kernel<L, W>), dim3(grid), dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((tdt_cells_kernel<L, W>), dim3(grid), dim3(256), 0, s, p);
        return hipGetLastError();
    });
}

hipError_t launch_tdt_cells(const TdtParams &p, hipStream_t s) {
    const bool vec = ((p.V + p.D) % 4 == 0) && (((uintptr_t)p.acts & 15) == 0);
    return vec ? launch_tdt_percell<false, 4>(p, s) : launch_tdt_percell<false, 1>(p, s);
}

hipError_t launch_tdt_grad(const TdtParams &p, hipStream_t s) {
    const bool vec = ((p.V + p.D) % 4 == 0) && ((((uintptr_t)p.acts | (uintptr_t)p.grads) & 15) == 0);
    return vec ? launch_tdt_percell<true, 4>(p, s) : launch_tdt_percell<true, 1>(p, s);
}

// ---------------------------------------------------------------------------------------------
// Sweeps.  Thread u owns lattice column u; step n visits the nodes (n - u, u).  Row n of alpha / beta goes to slot n % kTdtRing of the
// LDS ring (and to the workspace); a step reads the slots of rows n -+ 1 ... n -+ (dmax + 1), its own column for the blank edges and
// the neighbouring column for the label edges, and writes its own slot, which held row n -+ kTdtRing: the barrier at the end of a
// step orders this step's writes before the next step's reads AND the previous step's reads before this step's writes to the slot
// they no longer need.  An edge that does not exist gets the weight -inf, so its term drops out of the max and adds exp(-inf) = 0.
// ---------------------------------------------------------------------------------------------
struct TdtWeights {
    float wb[kTdtMaxD], wl[kTdtMaxD];
};

// the weights of the edges INTO node (n - u, u): those of its source cells (n - d_i - u, u) and (n - d_i - u, u - 1)
__device__ __forceinline__ void tdt_load_alpha(TdtWeights &x, const TdtParams &p, const float *w, const int n, const int u,
                                               const int Tb, const int Ub) {
    const int t = n - u, D = p.D;
    const size_t plane = (size_t)p.N * (size_t)p.Up;
    const bool node = u <= Ub && t >= 0 && (t < Tb || (t == Tb && u == Ub));
#pragma unroll
    for (int i = 0; i < kTdtMaxD; ++i) {
        x.wb[i] = x.wl[i] = -INFINITY;
        if (i < D) {
            const int d = p.dur[i];
            if (node && d > 0 && t - d >= 0) x.wb[i] = w[(size_t)i * plane + (size_t)(n - d) * (size_t)p.Up + u];
            if (node && u >= 1 && t < Tb && t - d >= 0) x.wl[i] = w[(size_t)(D + i) * plane + (size_t)(n - d - 1) * (size_t)p.Up + u - 1];
        }
    }
}

// the weights of the edges OUT OF cell (n - u, u): its own
__device__ __forceinline__ void tdt_load_beta(TdtWeights &x, const TdtParams &p, const float *w, const int n, const int u,
                                              const int Tb, const int Ub) {
    const int t = n - u, D = p.D;
    const size_t plane = (size_t)p.N * (size_t)p.Up;
    const bool live = u <= Ub && t >= 0 && t < Tb;
#pragma unroll
    for (int i = 0; i < kTdtMaxD; ++i) {
        x.wb[i] = x.wl[i] = -INFINITY;
        if (i < D) {
            const int d = p.dur[i];
            const size_t at = (size_t)n * (size_t)p.Up + u;
            if (live && d > 0 && (t + d < Tb || (t + d == Tb && u == Ub))) x.wb[i] = w[(size_t)i * plane + at];
            if (live && u < Ub && t + d < Tb) x.wl[i] = w[(size_t)(D + i) * plane + at];
        }
    }
}

template <bool BETA>
__device__ __forceinline__ void tdt_sweep(const TdtParams &p, double *ring) {
    const int b = blockIdx.x >> 1, u = threadIdx.x;
    int Tb = p.input_lengths[b], Ub = p.label_lengths[b];
    const bool bad = Tb < 1 || Tb > p.T || Ub < 0 || Ub > p.U - 1;
    Tb = min(max(Tb, 1), p.T);
    Ub = min(max(Ub, 0), p.U - 1);
    const int Up = p.Up, D = p.D;
    const int last = Tb + Ub;  // the terminal's row; last < N
    const size_t plane = (size_t)p.N * (size_t)Up;
    const float *w = p.w + (size_t)b * (size_t)(2 * D) * plane;
    double *out = (BETA ? p.beta : p.alpha) + (size_t)b * plane;
    const int side = BETA ? min(u + 1, Up - 1) : max(u - 1, 0);  // the column of the label edges' other end

#pragma unroll
    for (int r = 0; r < kTdtRing; ++r) ring[r * Up + u] = -INFINITY;
    __syncthreads();

    TdtWeights cur, nxt;
    if (BETA)
        tdt_load_beta(cur, p, w, last, u, Tb, Ub);
    else
        tdt_load_alpha(cur, p, w, 0, u, Tb, Ub);
    double v = -INFINITY;
    for (int s = 0; s <= last; ++s) {
        const int n = BETA ? last - s : s;
        if (s < last) {  // the next step's weights: in flight under this step's arithmetic
            if (BETA)
                tdt_load_beta(nxt, p, w, n - 1, u, Tb, Ub);
            else
                tdt_load_alpha(nxt, p, w, n + 1, u, Tb, Ub);
        }
        double tb[kTdtMaxD], tl[kTdtMaxD];
        double mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < kTdtMaxD; ++i) {
            if (i < D) {
                const int d = p.dur[i];
                // rows n -+ d and n -+ (d + 1); before the first / after the last row the ring still holds its -inf
                const int rb = BETA ? n + d : n - d + 2 * kTdtRing, rl = BETA ? n + d + 1 : n - d - 1 + 2 * kTdtRing;
                tb[i] = ring[(rb % kTdtRing) * Up + u] + (double)cur.wb[i];
                tl[i] = ring[(rl % kTdtRing) * Up + side] + (double)cur.wl[i];
                mx = fmax(mx, fmax(tb[i], tl[i]));
            }
        }
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i < kTdtMaxD; ++i) {
            if (i < D) {
                sum += __expf((float)(tb[i] - mx));  // (mx = -inf: NaN, not used)
                sum += __expf((float)(tl[i] - mx));
            }
        }
        v = mx == -INFINITY ? mx : mx + (double)__logf(sum);
        if (s == 0 && u == (BETA ? Ub : 0)) v = 0.0;  // alpha(0, 0) / beta(T_b, L_b)
        ring[(n % kTdtRing) * Up + u] = v;
        out[(size_t)n * (size_t)Up + u] = v;
        __syncthreads();
        cur = nxt;
    }

    if (!BETA && u == Ub) {  // ln P = alpha(T_b, L_b): -inf when no path exists
        const double lnP = bad ? (double)__int_as_float(0x7fc00000) : v;
        p.lnP[b] = lnP;
        if (p.costs) p.costs[b] = (float)(-lnP);
    }
}

__global__ void __launch_bounds__(kTdtMaxU) tdt_sweep_kernel(const TdtParams p) {
    // 80 KB, declared for maxU = 1024; a launch of Up threads uses kTdtRing * Up of it.  The static size holds a CU to two of these
    // workgroups whatever U is; the grid is 2B workgroups on 256 CUs, so that binds only beyond B = 256.  Dynamic LDS of
    // kTdtRing * Up doubles would lift it, at the price of raising the kernel's dynamic-LDS limit (above 64 KB) before the launch.
    __shared__ double ring[kTdtRing * kTdtMaxU];
    if (blockIdx.x & 1)
        tdt_sweep<true>(p, ring);
    else
        tdt_sweep<false>(p, ring);
}

hipError_t launch_tdt_sweeps(const TdtParams &p, hipStream_t s) {
    hipLaunchKernelGGL(tdt_sweep_kernel, dim3(2 * p.B), dim3(p.Up), 0, s, p);
    return hipGetLastError();
}

}  // namespace rnnt
