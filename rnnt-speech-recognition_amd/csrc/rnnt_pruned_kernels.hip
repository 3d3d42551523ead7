// rnnt_pruned_kernels.hip -- the PRUNED transducer loss: the lattice on a band of S symbols per frame, on the standard and on
// the modified topology (include/rnnt_pruned.h; rnnt_pruned.h for the workspace).
//
//   pruned_cells_kernel<L, W>    one read of the logits: log-softmax normaliser per PRESENT cell (f32, online max / sum, L lanes
//                                per cell, W = 4: 16-byte loads, W = 1: rows that are not 16-byte aligned), stored as {lpb, lpl}
//                                and lse per band slot.  Absent cells are skipped.
//   pruned_sweep_kernel<G, TOPO> ONE launch for both directions: the first half of the grid sweeps alpha, the second beta.  A
//                                lane is a band slot; a group of G lanes (the next power of two >= S) is one utterance, 64 / G
//                                utterances share a wavefront.  Row t's band begins at sb[t], the row before at any other place:
//                                the value of the same lattice column sits at slot s + sb[t] - sb[t -+ 1], fetched by a lane
//                                permute with an explicit range test.  The standard lattice adds the chain along the row (S - 1
//                                dependent log-adds), the modified one has no dependency inside a row.  float64 carry, the
//                                log(1 + e^-|d|) term on the float32 units; alpha and the backward edge terms stored as float64.
//   pruned_grad_kernel<L, W>     one write of EVERY element of grads: zeros for absent cells (not read), otherwise e_b, e_l from
//                                the slot's own alpha / edge terms and one pass over the V logits.
//
// An absent source is selected away BEFORE the addition, so neither the workspace's previous contents nor absent logits can
// enter a sum.  Every sum has an order fixed by V (cell pass) and by the utterance's own cells (sweeps): an utterance's results
// do not depend on the batch around it.
#include "rnnt_pruned.h"

#include <math.h>

#include <type_traits>

namespace rnnt {

constexpr float kPrunedNegInit = -3.0e38f;  // finite: two lanes without elements merge to (this, 0), not to NaN

struct PrunedCell {
    int b, t, s;
    int Tb, Lb;    // clamped into the tensor
    long long u;   // sb[t] + s: cannot overflow
    bool bad;      // out-of-range lengths: the utterance is reported as NaN
    bool present;  // t < T_b, 0 <= u <= L_b
};

__device__ __forceinline__ PrunedCell pruned_cell(const PrunedParams &p, const uint32_t c) {
    PrunedCell m;
    const uint32_t bt = c / (uint32_t)p.S;
    m.s = (int)(c - bt * (uint32_t)p.S);
    m.b = (int)(bt / (uint32_t)p.T);
    m.t = (int)(bt - (uint32_t)m.b * (uint32_t)p.T);
    const int Tb = p.input_lengths[m.b], Lb = p.label_lengths[m.b];
    m.bad = Tb < 1 || Tb > p.T || Lb < 0 || Lb > p.U - 1;
    m.Tb = min(max(Tb, 1), p.T);
    m.Lb = min(max(Lb, 0), p.U - 1);
    m.u = (long long)p.s_begin[bt] + (long long)m.s;
    m.present = m.t < m.Tb && m.u >= 0 && m.u <= (long long)m.Lb;
    return m;
}

// the W elements of a row that start at element i (W = 1: any alignment; W = 4: V % 4 == 0 and a 16-byte-aligned tensor)
template <int W>
__device__ __forceinline__ void pruned_load(float (&x)[W], const float *row, const int i) {
    if constexpr (W == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(row + i);
        x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
        x[0] = row[i];
    }
}
template <int W>
__device__ __forceinline__ void pruned_store(float *row, const int i, const float (&x)[W]) {
    if constexpr (W == 4)
        *reinterpret_cast<float4 *>(row + i) = make_float4(x[0], x[1], x[2], x[3]);
    else
        row[i] = x[0];
}

// ---------------------------------------------------------------------------------------------
// Cell pass.  A group of L lanes owns one band slot; lane j takes the pieces j, j + L, ... (W elements each) of its V logits and
// keeps a running (max, sum of exp(x - max)); the L partial pairs are merged by a butterfly.
// ---------------------------------------------------------------------------------------------
template <int L, int W>
__global__ void __launch_bounds__(256) pruned_cells_kernel(const PrunedParams p) {
    constexpr int kCellsPerBlock = 256 / L;
    const int tid = threadIdx.x;
    const int j = tid % L;
    const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.T * (uint32_t)p.S;
    const uint32_t c = blockIdx.x * (uint32_t)kCellsPerBlock + (uint32_t)(tid / L);
    if (c >= ncells) return;
    const PrunedCell m = pruned_cell(p, c);
    if (!m.present) return;  // absent: not read (the whole group leaves together)

    const int V = p.V;
    const float *row = p.acts + (size_t)c * (size_t)V;
    float mx = kPrunedNegInit, s = 0.0f;
#pragma unroll 2
    for (int i = j * W; i < V; i += L * W) {
        float x[W];
        pruned_load<W>(x, row, i);
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
    if (m.u < (long long)m.Lb) {
        int lab = p.labels[(size_t)m.b * (size_t)(p.U - 1) + (size_t)m.u];
        lab = min(max(lab, 0), V - 1);
        out.y = row[lab] - lse;
    }
    p.lp[c] = out;
    p.lse[c] = lse;
}

// ---------------------------------------------------------------------------------------------
// Gradient pass: the same lane map.  With e_b = exp(alpha + edge.x - ln P), e_l = exp(alpha + edge.y - ln P):
//   grads[v] = cost_scale ((e_b + e_l + lambda e_l) softmax[v] - [v == blank] e_b - [v == y_u] (1 + lambda) e_l)
// ---------------------------------------------------------------------------------------------
template <int L, int W>
__global__ void __launch_bounds__(256) pruned_grad_kernel(const PrunedParams p) {
    constexpr int kCellsPerBlock = 256 / L;
    const int tid = threadIdx.x;
    const int j = tid % L;
    const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.T * (uint32_t)p.S;
    const uint32_t c = blockIdx.x * (uint32_t)kCellsPerBlock + (uint32_t)(tid / L);
    if (c >= ncells) return;
    const PrunedCell m = pruned_cell(p, c);
    const int V = p.V;
    float *grow = p.grads + (size_t)c * (size_t)V;
    const double lnP = p.lnP[m.b];  // NaN for out-of-range lengths
    if (!m.present || (!m.bad && lnP == -INFINITY)) {  // exact zeros; the logits are not read
        float z[W];
#pragma unroll
        for (int k = 0; k < W; ++k) z[k] = 0.0f;
        for (int i = j * W; i < V; i += L * W) pruned_store<W>(grow, i, z);
        return;
    }
    if (m.bad) {
        float z[W];
#pragma unroll
        for (int k = 0; k < W; ++k) z[k] = __int_as_float(0x7fc00000);
        for (int i = j * W; i < V; i += L * W) pruned_store<W>(grow, i, z);
        return;
    }
    const double a = p.alpha[c];
    const double2 ed = p.edge[c];
    const float eb = __expf((float)(a + ed.x - lnP));  // (-inf: 0)
    float el = 0.0f;
    int lab = -1;
    if (m.u < (long long)m.Lb) {
        el = __expf((float)(a + ed.y - lnP));
        lab = p.labels[(size_t)m.b * (size_t)(p.U - 1) + (size_t)m.u];
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
        pruned_load<W>(x, row, i);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            float g = coef * __expf(x[k] - lse);
            g -= (i + k == p.blank) ? sb : 0.0f;
            g -= (i + k == lab) ? sl : 0.0f;
            x[k] = g;
        }
        pruned_store<W>(grow, i, x);
    }
}

// lanes per cell: the smallest power of two that gives every piece of a row a lane, at most one wavefront
template <int W, typename F>
static hipError_t pruned_dispatch_L(const int V, F &&f) {
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
static hipError_t launch_pruned_percell(const PrunedParams &p, hipStream_t s) {
    return pruned_dispatch_L<W>(p.V, [&](auto l) {
        constexpr int L = decltype(l)::value;
        const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.T * (uint32_t)p.S;
        const uint32_t per = 256 / L;
        const uint32_t grid = (ncells + per - 1) / per;
        if (GRAD)
            hipLaunchKernelGGL((pruned_grad_kernel<L, W>), dim3(grid), dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((pruned_cells_kernel<L, W>), dim3(grid), dim3(256), 0, s, p);
        return hipGetLastError();
    });
}

hipError_t launch_pruned_cells(const PrunedParams &p, hipStream_t s) {
    const bool vec = (p.V % 4 == 0) && (((uintptr_t)p.acts & 15) == 0);
    return vec ? launch_pruned_percell<false, 4>(p, s) : launch_pruned_percell<false, 1>(p, s);
}

hipError_t launch_pruned_grad(const PrunedParams &p, hipStream_t s) {
    const bool vec = (p.V % 4 == 0) && ((((uintptr_t)p.acts | (uintptr_t)p.grads) & 15) == 0);
    return vec ? launch_pruned_percell<true, 4>(p, s) : launch_pruned_percell<true, 1>(p, s);
}

// ---------------------------------------------------------------------------------------------
// Sweeps.
// ---------------------------------------------------------------------------------------------
constexpr double kNegInf = -INFINITY;

// log(e^x + e^y): float64 carry, the term in (0, ln 2] on the float32 units (include/rnnt.h, Numerics)
__device__ __forceinline__ double pruned_logadd(const double x, const double y) {
    const double hi = fmax(x, y), lo = fmin(x, y);
    const float d = (float)(lo - hi);  // <= 0 (NaN when both are -inf: the result is taken from hi)
    const float term = __logf(1.0f + __expf(d));
    return hi == kNegInf ? hi : hi + (double)term;
}

// lane `src`'s value of v (every lane of the wavefront executes this); -inf unless `ok`
__device__ __forceinline__ double pruned_fetch(const double v, const int src, const bool ok) {
    const double r = __shfl(v, src & 63, 64);
    return ok ? r : kNegInf;
}

constexpr int kPrunedRows = 4;  // rows of {lpb, lpl} and of sb in flight per buffer, ahead of the chain

struct PrunedRow {
    float2 e;
    int sb;
};

template <int G, int TOPO, bool BETA>
__device__ __forceinline__ void pruned_sweep(const PrunedParams &p, const int blk) {
    constexpr int kPer = 64 / G;  // utterances per wavefront
    const int lane = threadIdx.x;
    const int grp = lane / G, s = lane % G, gbase = grp * G;
    const int S = p.S;
    const int job = blk * kPer + grp;
    const bool live = job < p.B;  // (the last wavefront of a batch may be partial: its spare groups run along and store nothing)
    const int b = min(job, p.B - 1);
    int Tb = p.input_lengths[b], Lb = p.label_lengths[b];
    const bool bad = Tb < 1 || Tb > p.T || Lb < 0 || Lb > p.U - 1;
    Tb = min(max(Tb, 1), p.T);
    Lb = min(max(Lb, 0), p.U - 1);
    const bool slot_ok = s < S;
    const size_t base = (size_t)b * (size_t)p.T * (size_t)S;
    const float2 *lp = p.lp + base + min(s, S - 1);
    const int *sbp = p.s_begin + (size_t)b * (size_t)p.T;
    const int steps = live ? Tb : 0;
    int nsteps = steps;  // the wavefront's trip count: every lane runs every step, so that every permute finds its source
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) nsteps = max(nsteps, __shfl_xor(nsteps, off, 64));

    // the state a row hands to the next one, by slot: -inf for absent cells
    double carry0 = kNegInf;  // alpha: alpha + lpb;  beta: beta
    double carry1 = kNegInf;  // modified alpha: alpha + lpl
    long long sb_prev = 0;
    double fin0 = kNegInf, fin1 = kNegInf;  // alpha: the terms of ln P, left by the last row

    int ls = 0;  // the next step to load: step i works on lattice row i (alpha) / T_b - 1 - i (beta)
    auto load_block = [&](PrunedRow(&buf)[kPrunedRows]) {
#pragma unroll
        for (int g = 0; g < kPrunedRows; ++g) {
            const int i = min(ls, Tb - 1);  // (past the end: a row of this utterance again, not used)
            const int t = BETA ? Tb - 1 - i : i;
            buf[g].e = lp[(size_t)t * S];
            buf[g].sb = sbp[t];
            ++ls;
        }
    };
    auto step = [&](const int i, const PrunedRow &d) {
        const bool active = i < steps;
        const int t = BETA ? Tb - 1 - i : i;
        const long long sbt = d.sb;
        const long long u = sbt + s;
        const bool present = active && slot_ok && u >= 0 && u <= (long long)Lb;
        const bool has_label = present && u < (long long)Lb;
        const double lpb = present ? (double)d.e.x : 0.0;    // selected before any addition: what an absent slot of the
        const double lpl = has_label ? (double)d.e.y : 0.0;  // workspace holds never enters a sum
        // the slot of the same lattice column in the row before (in sweep order)
        const long long src = (long long)s + sbt - sb_prev;
        const bool first = i == 0;
        const bool ok0 = !first && src >= 0 && src < S;
        const size_t at = base + (size_t)t * S + s;
        if constexpr (!BETA) {
            double a;
            if constexpr (TOPO == 0) {
                const double below = pruned_fetch(carry0, gbase + (int)(ok0 ? src : 0), ok0);
                const double x = (first && u == 0) ? 0.0 : below;
                a = present ? x : kNegInf;
                for (int k = 1; k < S; ++k) {  // the chain along the row: alpha(t,u-1) + lpl(t,u-1) -> alpha(t,u)
                    const double right = has_label ? a + lpl : kNegInf;
                    const double left = __shfl(right, (lane - 1) & 63, 64);
                    if (s == k && present) a = pruned_logadd(x, left);
                }
            } else {
                const bool ok1 = !first && src - 1 >= 0 && src - 1 < S;
                const double below = pruned_fetch(carry0, gbase + (int)(ok0 ? src : 0), ok0);
                const double diag = pruned_fetch(carry1, gbase + (int)(ok1 ? src - 1 : 0), ok1);
                const double x = first ? (u == 0 ? 0.0 : kNegInf) : pruned_logadd(below, diag);
                a = present ? x : kNegInf;
            }
            if (active && slot_ok) p.alpha[at] = a;
            if (active) {
                carry0 = present ? a + lpb : kNegInf;
                carry1 = has_label ? a + lpl : kNegInf;
                sb_prev = sbt;
                if (i == steps - 1) {
                    fin0 = (present && u == (long long)Lb) ? carry0 : kNegInf;
                    fin1 = (TOPO == 1 && has_label && u == (long long)Lb - 1) ? carry1 : kNegInf;
                }
            }
        } else {
            double bb, bl, beta;
            if constexpr (TOPO == 0) {
                const double up = pruned_fetch(carry0, gbase + (int)(ok0 ? src : 0), ok0);
                bb = present ? lpb + up : kNegInf;
                if (first && present && u == (long long)Lb) bb = lpb;  // the final blank
                bl = kNegInf;
                beta = bb;
                for (int k = S - 2; k >= 0; --k) {  // the chain along the row: beta(t,u+1) -> beta(t,u)
                    const double right = __shfl(beta, (lane + 1) & 63, 64);
                    if (s == k && has_label) {
                        bl = lpl + right;
                        beta = pruned_logadd(bb, bl);
                    }
                }
            } else {
                const bool ok1 = !first && src + 1 >= 0 && src + 1 < S;
                double up = pruned_fetch(carry0, gbase + (int)(ok0 ? src : 0), ok0);
                double upr = pruned_fetch(carry0, gbase + (int)(ok1 ? src + 1 : 0), ok1);
                if (first) {  // the row of the end node (T_b, L_b)
                    up = u == (long long)Lb ? 0.0 : kNegInf;
                    upr = u + 1 == (long long)Lb ? 0.0 : kNegInf;
                }
                bb = present ? lpb + up : kNegInf;
                bl = has_label ? lpl + upr : kNegInf;
                beta = pruned_logadd(bb, bl);
            }
            if (active && slot_ok) p.edge[at] = make_double2(bb, bl);
            if (active) {
                carry0 = present ? beta : kNegInf;
                sb_prev = sbt;
            }
        }
    };

    PrunedRow bufA[kPrunedRows], bufB[kPrunedRows];
    load_block(bufA);
    for (int i0 = 0; i0 < nsteps; i0 += 2 * kPrunedRows) {
        load_block(bufB);
#pragma unroll
        for (int g = 0; g < kPrunedRows; ++g)
            if (i0 + g < nsteps) step(i0 + g, bufA[g]);
        load_block(bufA);
#pragma unroll
        for (int g = 0; g < kPrunedRows; ++g)
            if (i0 + kPrunedRows + g < nsteps) step(i0 + kPrunedRows + g, bufB[g]);
    }

    if constexpr (!BETA) {  // ln P: at most one slot of the last row holds each term; -inf when the band does not reach the end
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) {
            fin0 = fmax(fin0, __shfl_xor(fin0, off, 64));
            fin1 = fmax(fin1, __shfl_xor(fin1, off, 64));
        }
        if (live && s == 0) {
            const double ll = TOPO == 1 ? pruned_logadd(fin0, fin1) : fin0;
            const double lnP = bad ? (double)__int_as_float(0x7fc00000) : ll;
            p.lnP[b] = lnP;
            if (p.costs) p.costs[b] = (float)(-lnP);
        }
    }
}

template <int G, int TOPO>
__global__ void __launch_bounds__(64) pruned_sweep_kernel(const PrunedParams p, const int nblk) {
    if ((int)blockIdx.x >= nblk)
        pruned_sweep<G, TOPO, true>(p, (int)blockIdx.x - nblk);
    else
        pruned_sweep<G, TOPO, false>(p, (int)blockIdx.x);
}

template <int G>
static hipError_t launch_sweep_G(const PrunedParams &p, hipStream_t s) {
    const int per = 64 / G;
    const int nblk = (p.B + per - 1) / per;
    if (p.topology == 0)
        hipLaunchKernelGGL((pruned_sweep_kernel<G, 0>), dim3(2 * nblk), dim3(64), 0, s, p, nblk);
    else
        hipLaunchKernelGGL((pruned_sweep_kernel<G, 1>), dim3(2 * nblk), dim3(64), 0, s, p, nblk);
    return hipGetLastError();
}

hipError_t launch_pruned_sweeps(const PrunedParams &p, hipStream_t s) {
    // lanes per utterance: the next power of two >= S
    if (p.S <= 1) return launch_sweep_G<1>(p, s);
    if (p.S <= 2) return launch_sweep_G<2>(p, s);
    if (p.S <= 4) return launch_sweep_G<4>(p, s);
    if (p.S <= 8) return launch_sweep_G<8>(p, s);
    if (p.S <= 16) return launch_sweep_G<16>(p, s);
    if (p.S <= 32) return launch_sweep_G<32>(p, s);
    return launch_sweep_G<64>(p, s);
}

}  // namespace rnnt
