// rnnt_simple_kernels.hip -- the SIMPLE transducer loss: an additive joiner, logit(t, u, v) = am[t, v] + lm[u, v], on the standard
// and on the modified lattice (include/rnnt_simple.h; rnnt_simple.h for the skewed lattice arrays and the workspace; DESIGN.md
// section 8p).  The [B, T, U, V] tensor is never formed: every pass re-evaluates am + lm from the two small inputs.
//
//   simple_rows_kernel            Za(t) = ln sum_v exp(am[t, v]) and Zl(u) likewise: one wavefront per live row.
//   simple_cells_kernel           a workgroup owns 32 x 32 lattice cells of one utterance (a thread: 2 x 2); its am and lm rows are
//                                 staged in LDS 64 symbols at a time; Z(t, u) by an online max / sum over V with the CELL'S OWN
//                                 maximum (every exponential is at most 1: am and lm may peak at different symbols).  Writes Z and
//                                 {lpb, lpl} per present cell.
//   simple_sweep_kernel<K, G, W>  ONE launch for both directions and one kernel shape for both lattices: workgroup 2b sweeps alpha,
//                                 2b + 1 beta of utterance b over the rows n = t + skew u.  Lanes map to lattice columns (K per
//                                 thread); float64 carry, the log(1 + e^-|d|) term of a log-add on the float32 units; alpha and beta
//                                 stored as float64.  One wavefront up to 1024 columns (the neighbour's column by DPP), 1024 threads
//                                 beyond (through LDS, one barrier per row).
//   simple_occupancy_kernel       {e_b, e_l} of every cell, and occupancy = e_b + e_l where the caller asks for it.
//   simple_grad_am_kernel<VL>     a thread owns one symbol of 4 frames and runs over u = 0 ... L_b in that order;
//   simple_grad_lm_kernel<VL>     a thread owns one symbol of 4 columns and runs over t = 0 ... T_b - 1 in that order.
//
// No atomics: every sum has an order fixed by V (rows, cells) or by the utterance's own cells (sweeps, gradients), so an
// utterance's results do not depend on the batch around it and two calls give the same bits.
#include "rnnt_simple.h"

#include <math.h>

namespace rnnt {

constexpr float kSimpleNegInit = -3.0e38f;  // finite: a running maximum that has seen nothing rescales a zero sum by exp(-huge) = 0
constexpr int kSimpleTile = 32;             // lattice cells per workgroup: kSimpleTile x kSimpleTile
constexpr int kSimpleChunk = 64;            // symbols staged in LDS at a time
constexpr int kSimpleSub = 16;              // symbols held in registers at a time

struct SimpleLens {
    int Tb, Lb;  // clamped into the tensors
    bool bad;    // out-of-range lengths: the utterance is reported as NaN
};

__device__ __forceinline__ SimpleLens simple_lens(const SimpleParams &p, const int b) {
    SimpleLens m;
    const int Tb = p.input_lengths[b], Lb = p.label_lengths[b];
    m.bad = Tb < 1 || Tb > p.T || Lb < 0 || Lb > p.U - 1;
    m.Tb = min(max(Tb, 1), p.T);
    m.Lb = min(max(Lb, 0), p.U - 1);
    return m;
}

__device__ __forceinline__ float simple_nan() { return __int_as_float(0x7fc00000); }

// ---------------------------------------------------------------------------------------------
// Row normalisers: wavefront r of the grid owns row r of am (r < B T) or row r - B T of lm.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) simple_rows_kernel(const SimpleParams p) {
    const int lane = threadIdx.x & 63;
    const uint32_t nam = (uint32_t)p.B * (uint32_t)p.T, nlm = (uint32_t)p.B * (uint32_t)p.U;
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= nam + nlm) return;
    const float *row;
    float *out;
    if (r < nam) {
        const int b = (int)(r / (uint32_t)p.T), t = (int)(r - (uint32_t)b * (uint32_t)p.T);
        if (t >= simple_lens(p, b).Tb) return;  // padded: not read
        row = p.am + (size_t)r * (size_t)p.V;
        out = p.Za + r;
    } else {
        const uint32_t q = r - nam;
        const int b = (int)(q / (uint32_t)p.U), u = (int)(q - (uint32_t)b * (uint32_t)p.U);
        if (u > simple_lens(p, b).Lb) return;
        row = p.lm + (size_t)q * (size_t)p.V;
        out = p.Zl + q;
    }
    float mx = kSimpleNegInit;
    for (int i = lane; i < p.V; i += 64) mx = fmaxf(mx, row[i]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    float s = 0.0f;
    for (int i = lane; i < p.V; i += 64) s += __expf(row[i] - mx);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);  // (a + b on both sides of a pair: the same bits in every lane)
    if (lane == 0) *out = mx + __logf(s);
}

// ---------------------------------------------------------------------------------------------
// Cell pass.  Thread (tx, ty) of a 16 x 16 workgroup owns the cells (t0 + 2 ty + i, u0 + 2 tx + j), i, j in {0, 1}.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) simple_cells_kernel(const SimpleParams p, const int tiles_t, const int tiles_u) {
    __shared__ float am_s[kSimpleTile][kSimpleChunk + 1];
    __shared__ float lm_s[kSimpleTile][kSimpleChunk + 1];
    const int tid = threadIdx.x;
    const uint32_t per = (uint32_t)tiles_t * (uint32_t)tiles_u;
    const int b = (int)(blockIdx.x / per);
    const uint32_t rem = blockIdx.x - (uint32_t)b * per;
    const int t0 = (int)(rem / (uint32_t)tiles_u) * kSimpleTile, u0 = (int)(rem % (uint32_t)tiles_u) * kSimpleTile;
    const SimpleLens m = simple_lens(p, b);
    if (t0 >= m.Tb || u0 > m.Lb) return;  // no present cell in the tile (the whole workgroup leaves together)
    const int V = p.V;
    const int tx = tid & 15, ty = tid >> 4;
    const float *amb = p.am + (size_t)b * p.T * (size_t)V;
    const float *lmb = p.lm + (size_t)b * p.U * (size_t)V;

    float mx[2][2], sm[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) mx[i][j] = kSimpleNegInit, sm[i][j] = 0.0f;

    for (int c0 = 0; c0 < V; c0 += kSimpleChunk) {
        __syncthreads();
        for (int idx = tid; idx < kSimpleTile * kSimpleChunk; idx += 256) {
            const int r = idx / kSimpleChunk, v = c0 + idx % kSimpleChunk;
            // rows past the utterance are never read (zeros); symbols past V: -inf on one side, so that exp(x - max) = 0
            am_s[r][idx % kSimpleChunk] = v < V ? (t0 + r < m.Tb ? amb[(size_t)(t0 + r) * V + v] : 0.0f) : -INFINITY;
            lm_s[r][idx % kSimpleChunk] = (v < V && u0 + r <= m.Lb) ? lmb[(size_t)(u0 + r) * V + v] : 0.0f;
        }
        __syncthreads();
        for (int s0 = 0; s0 < kSimpleChunk && c0 + s0 < V; s0 += kSimpleSub) {
            float a[2][kSimpleSub], l[2][kSimpleSub];
#pragma unroll
            for (int k = 0; k < kSimpleSub; ++k) {
                a[0][k] = am_s[2 * ty][s0 + k], a[1][k] = am_s[2 * ty + 1][s0 + k];
                l[0][k] = lm_s[2 * tx][s0 + k], l[1][k] = lm_s[2 * tx + 1][s0 + k];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float nm = mx[i][j];
#pragma unroll
                    for (int k = 0; k < kSimpleSub; ++k) nm = fmaxf(nm, a[i][k] + l[j][k]);
                    float e = 0.0f;
#pragma unroll
                    for (int k = 0; k < kSimpleSub; ++k) e += __expf((a[i][k] + l[j][k]) - nm);
                    sm[i][j] = sm[i][j] * __expf(mx[i][j] - nm) + e;
                    mx[i][j] = nm;
                }
        }
    }

    const float ws = p.w_scale, as = p.a_scale, ls = p.l_scale;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int t = t0 + 2 * ty + i, u = u0 + 2 * tx + j;
            if (t >= m.Tb || u > m.Lb) continue;
            const float Z = mx[i][j] + __logf(sm[i][j]);
            const float *ar = amb + (size_t)t * V, *lr = lmb + (size_t)u * V;
            const float za = p.Za[(size_t)b * p.T + t], zl = p.Zl[(size_t)b * p.U + u];
            auto lp = [&](const int v) { return ws * ((ar[v] + lr[v]) - Z) + as * (ar[v] - za) + ls * (lr[v] - zl); };
            float2 out;
            out.x = lp(p.blank);
            out.y = 0.0f;
            if (u < m.Lb) {
                int lab = p.labels[(size_t)b * (size_t)(p.U - 1) + u];
                lab = min(max(lab, 0), V - 1);
                out.y = lp(lab);
            }
            p.Z[((size_t)b * p.T + t) * (size_t)p.U + u] = Z;
            p.lp[((size_t)b * p.NR + t + p.skew * u) * (size_t)p.Up + u] = out;
        }
}

// ---------------------------------------------------------------------------------------------
// Sweeps.  Thread j owns the lattice columns j K ... j K + K - 1; only the edge column's value crosses to the neighbouring thread
// (a whole-wave DPP shift, or LDS + one barrier per row in the wide kernel).  Nodes that are not valid are -inf and the {lpb, lpl}
// at their place (never written by the cell pass) are selected away before the addition.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double simple_dpp(const double x, const double fill, const bool from_lower) {
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
__device__ __forceinline__ double simple_logadd(const double x, const double y) {
    const double hi = fmax(x, y), lo = fmin(x, y);
    const float d = (float)(lo - hi);  // <= 0 (NaN when both are -inf: the result is taken from hi)
    const float term = __logf(1.0f + __expf(d));
    return hi == -INFINITY ? hi : hi + (double)term;
}

template <int K>
struct SimpleRow {
    float2 e[K];
};

template <int K>
__device__ __forceinline__ void simple_load_row(SimpleRow<K> &d, const float2 *rowp) {
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
__device__ __forceinline__ void simple_store_row(double *rowp, const double (&v)[K]) {
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
__device__ __forceinline__ void simple_sweep(const SimpleParams &p, double *xch) {
    constexpr int kThreads = WIDE ? 1024 : 64;
    const int b = blockIdx.x >> 1, tid = threadIdx.x;
    const SimpleLens m = simple_lens(p, b);
    const int Tb = m.Tb, Lb = m.Lb, skew = p.skew;
    const int nsteps = Tb + skew * Lb;  // rows 0 ... nsteps - 1 hold cells; row nsteps is the end node (T_b, L_b) alone
    const int Up = p.Up;
    const int u0 = tid * K;
    const float2 *lp = p.lp + (size_t)b * p.NR * (size_t)Up + u0;
    double *out = (BETA ? p.beta + (size_t)b * (p.NR + 1) * (size_t)Up : p.alpha + (size_t)b * p.NR * (size_t)Up) + u0;
    auto is_cell = [&](const int n, const int u) {
        const int t = n - skew * u;
        return t >= 0 && t < Tb && u <= Lb;
    };
    auto is_node = [&](const int n, const int u) { return is_cell(n, u) || (n == nsteps && u == Lb); };

    double v[K];  // alpha(row 0) / beta(row nsteps)
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (u0 + k == (BETA ? Lb : 0)) ? 0.0 : -INFINITY;
    if (BETA) simple_store_row<K>(out + (size_t)nsteps * Up, v);

    int ls = 0;  // the next step to load: step s reads row s (alpha) / nsteps - 1 - s (beta)
    auto load_block = [&](SimpleRow<K>(&buf)[G]) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int s = min(ls, nsteps - 1);  // (past the end: a row of this utterance again, not used)
            simple_load_row<K>(buf[g], lp + (size_t)(BETA ? nsteps - 1 - s : s) * Up);
            ++ls;
        }
    };
    auto step = [&](const int s, const SimpleRow<K> &d) {
        const int n = BETA ? nsteps - 1 - s : s;  // the row of the edges: lane u of row n -> lanes u and u + 1 of row n + 1
        double stay[K], move[K];
        if constexpr (!BETA) {
            simple_store_row<K>(out + (size_t)n * Up, v);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int u = u0 + k;
                const bool ok = is_cell(n, u);
                stay[k] = v[k] + (double)(ok ? d.e[k].x : 0.0f);
                move[k] = v[k] + (double)((ok && u < Lb) ? d.e[k].y : 0.0f);
            }
            double cin;
            if constexpr (WIDE) {
                double *x = xch + (s & 1) * kThreads;
                x[tid] = move[K - 1];
                __syncthreads();
                cin = tid ? x[tid - 1] : -INFINITY;
            } else {
                cin = simple_dpp(move[K - 1], -INFINITY, true);
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double from = k ? move[k - 1] : cin;
                v[k] = is_node(n + 1, u0 + k) ? simple_logadd(stay[k], from) : -INFINITY;
            }
        } else {
            double cin;
            if constexpr (WIDE) {
                double *x = xch + (s & 1) * kThreads;
                x[tid] = v[0];
                __syncthreads();
                cin = tid + 1 < kThreads ? x[tid + 1] : -INFINITY;
            } else {
                cin = simple_dpp(v[0], -INFINITY, false);
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int u = u0 + k;
                const bool ok = is_cell(n, u);
                stay[k] = v[k] + (double)(ok ? d.e[k].x : 0.0f);
                move[k] = (k + 1 < K ? v[k + 1] : cin) + (double)((ok && u < Lb) ? d.e[k].y : 0.0f);
            }
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = is_cell(n, u0 + k) ? simple_logadd(stay[k], move[k]) : -INFINITY;
            simple_store_row<K>(out + (size_t)n * Up, v);
        }
    };

    SimpleRow<K> bufA[G], bufB[G];
    load_block(bufA);
    for (int s0 = 0; s0 < nsteps; s0 += 2 * G) {
        load_block(bufB);
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (s0 + g < nsteps) step(s0 + g, bufA[g]);
        load_block(bufA);
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (s0 + G + g < nsteps) step(s0 + G + g, bufB[g]);
    }

    if constexpr (!BETA) {  // ln P = alpha(end node): -inf when no path exists (modified, L_b > T_b)
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (u0 + k == Lb) {
                const double lnP = m.bad ? (double)simple_nan() : v[k];
                p.lnP[b] = lnP;
                if (p.costs) p.costs[b] = (float)(-lnP);
            }
    }
}

template <int K, int G, bool WIDE>
__global__ void __launch_bounds__(WIDE ? 1024 : 64) simple_sweep_kernel(const SimpleParams p) {
    __shared__ double xch[WIDE ? 2 * 1024 : 2];  // the wide kernel's neighbour exchange, double-buffered by step parity
    if (blockIdx.x & 1)
        simple_sweep<K, G, WIDE, true>(p, xch);
    else
        simple_sweep<K, G, WIDE, false>(p, xch);
}

template <int K, int G, bool WIDE>
static hipError_t launch_simple_sweep_KG(const SimpleParams &p, hipStream_t s) {
    hipLaunchKernelGGL((simple_sweep_kernel<K, G, WIDE>), dim3(2 * p.B), dim3(WIDE ? 1024 : 64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_simple_sweeps(const SimpleParams &p, hipStream_t s) {
    // rows in flight per buffer: about 32 cells of registers per thread and buffer
    switch (sweep_K(p.U)) {
        case 1: return launch_simple_sweep_KG<1, 16, false>(p, s);
        case 2: return launch_simple_sweep_KG<2, 16, false>(p, s);
        case 3: return launch_simple_sweep_KG<3, 8, false>(p, s);
        case 4: return launch_simple_sweep_KG<4, 8, false>(p, s);
        case 6: return launch_simple_sweep_KG<6, 4, false>(p, s);
        case 8: return launch_simple_sweep_KG<8, 4, false>(p, s);
        case 12: return launch_simple_sweep_KG<12, 2, false>(p, s);
        case 16: return launch_simple_sweep_KG<16, 2, false>(p, s);
        default: break;
    }
    switch (align_wide_K(p.U)) {  // more than 1024 columns: 1024 threads
        case 2: return launch_simple_sweep_KG<2, 2, true>(p, s);
        case 3: return launch_simple_sweep_KG<3, 2, true>(p, s);
        case 4: return launch_simple_sweep_KG<4, 1, true>(p, s);
        case 6: return launch_simple_sweep_KG<6, 1, true>(p, s);
        case 8: return launch_simple_sweep_KG<8, 1, true>(p, s);
        default: return hipErrorInvalidValue;
    }
}

// ---------------------------------------------------------------------------------------------
// Occupancies: one thread per element of [B][T][U].
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) simple_occupancy_kernel(const SimpleParams p) {
    const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.T * (uint32_t)p.U;
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= ncells) return;
    const uint32_t bt = c / (uint32_t)p.U;
    const int u = (int)(c - bt * (uint32_t)p.U);
    const int b = (int)(bt / (uint32_t)p.T), t = (int)(bt - (uint32_t)b * (uint32_t)p.T);
    const SimpleLens m = simple_lens(p, b);
    float eb = 0.0f, el = 0.0f;
    if (t < m.Tb && u <= m.Lb) {
        const double lnP = p.lnP[b];
        if (m.bad) {
            eb = el = simple_nan();
        } else if (lnP != -INFINITY) {
            const int n = t + p.skew * u;
            const size_t at = ((size_t)b * p.NR + n) * (size_t)p.Up + u;
            const size_t nx = ((size_t)b * (p.NR + 1) + n + 1) * (size_t)p.Up + u;
            const double a = p.alpha[at];
            const float2 lp = p.lp[at];
            eb = __expf((float)(a + (double)lp.x + p.beta[nx] - lnP));
            if (u < m.Lb) el = __expf((float)(a + (double)lp.y + p.beta[nx + 1] - lnP));
        }
    }
    p.e[c] = make_float2(eb, el);
    if (p.occupancy) p.occupancy[c] = eb + el;
}

// ---------------------------------------------------------------------------------------------
// Gradient passes.  With occ = e_b + e_l and sj = exp(am + lm - Z) (at most 1 up to rounding):
//   grad_am[t, v] = cs (w sum_u occ sj + a exp(am - Za) sum_u occ - (w + a) ([v == blank] sum_u e_b + sum_{u: y_u == v} e_l))
//   grad_lm[u, v] = cs (w sum_t occ sj + l exp(lm - Zl) sum_t occ - (w + l) ([v == blank] sum_t e_b + [v == y_u] sum_t e_l))
// A thread owns symbol v of kSimpleR rows and adds in the order of the other index; VL lanes of a workgroup run along v.
// ---------------------------------------------------------------------------------------------
constexpr int kSimpleR = 4;

template <int VL>
__global__ void __launch_bounds__(256) simple_grad_am_kernel(const SimpleParams p, const int nv, const int nr) {
    constexpr int kRows = (256 / VL) * kSimpleR;
    const uint32_t per = (uint32_t)nv * (uint32_t)nr;
    const int b = (int)(blockIdx.x / per);
    const uint32_t rem = blockIdx.x - (uint32_t)b * per;
    const int v = (int)(rem % (uint32_t)nv) * VL + (int)(threadIdx.x % VL);
    const int t0 = (int)(rem / (uint32_t)nv) * kRows + (int)(threadIdx.x / VL) * kSimpleR;
    const int V = p.V, T = p.T, U = p.U;
    if (v >= V || t0 >= T) return;
    const SimpleLens m = simple_lens(p, b);
    const double lnP = p.lnP[b];
    float *g = p.grad_am + ((size_t)b * T + t0) * (size_t)V + v;
    if (t0 >= m.Tb || m.bad || lnP == -INFINITY) {  // padded rows and an utterance without a path: exact zeros, nothing is read
#pragma unroll
        for (int r = 0; r < kSimpleR; ++r)
            if (t0 + r < T) g[(size_t)r * V] = (m.bad && t0 + r < m.Tb) ? simple_nan() : 0.0f;
        return;
    }
    int tr[kSimpleR];  // (a row past T_b computes its last live neighbour again and stores a zero)
    float amv[kSimpleR], acc[kSimpleR], occs[kSimpleR], ebs[kSimpleR], els[kSimpleR];
#pragma unroll
    for (int r = 0; r < kSimpleR; ++r) {
        tr[r] = min(t0 + r, m.Tb - 1);
        amv[r] = p.am[((size_t)b * T + tr[r]) * (size_t)V + v];
        acc[r] = occs[r] = ebs[r] = els[r] = 0.0f;
    }
    const float *lmp = p.lm + (size_t)b * U * (size_t)V + v;
    const int *lab = p.labels + (size_t)b * (size_t)(U - 1);
    for (int u = 0; u <= m.Lb; ++u) {
        const float lmv = lmp[(size_t)u * V];
        const bool mine = u < m.Lb && min(max(lab[u], 0), V - 1) == v;
#pragma unroll
        for (int r = 0; r < kSimpleR; ++r) {
            const size_t c = ((size_t)b * T + tr[r]) * (size_t)U + u;
            const float2 e = p.e[c];
            const float occ = e.x + e.y;
            acc[r] += occ * __expf((amv[r] + lmv) - p.Z[c]);
            occs[r] += occ;
            ebs[r] += e.x;
            els[r] += mine ? e.y : 0.0f;
        }
    }
    const float cs = p.cost_scale ? p.cost_scale[b] : 1.0f;
#pragma unroll
    for (int r = 0; r < kSimpleR; ++r) {
        if (t0 + r >= T) break;
        const float sa = __expf(amv[r] - p.Za[(size_t)b * T + tr[r]]);
        const float eps = (v == p.blank ? ebs[r] : 0.0f) + els[r];
        const float x = cs * (p.w_scale * acc[r] + p.a_scale * (sa * occs[r]) - (p.w_scale + p.a_scale) * eps);
        g[(size_t)r * V] = t0 + r < m.Tb ? x : 0.0f;
    }
}

template <int VL>
__global__ void __launch_bounds__(256) simple_grad_lm_kernel(const SimpleParams p, const int nv, const int nr) {
    constexpr int kRows = (256 / VL) * kSimpleR;
    const uint32_t per = (uint32_t)nv * (uint32_t)nr;
    const int b = (int)(blockIdx.x / per);
    const uint32_t rem = blockIdx.x - (uint32_t)b * per;
    const int v = (int)(rem % (uint32_t)nv) * VL + (int)(threadIdx.x % VL);
    const int u0 = (int)(rem / (uint32_t)nv) * kRows + (int)(threadIdx.x / VL) * kSimpleR;
    const int V = p.V, T = p.T, U = p.U;
    if (v >= V || u0 >= U) return;
    const SimpleLens m = simple_lens(p, b);
    const double lnP = p.lnP[b];
    float *g = p.grad_lm + ((size_t)b * U + u0) * (size_t)V + v;
    if (u0 > m.Lb || m.bad || lnP == -INFINITY) {
#pragma unroll
        for (int r = 0; r < kSimpleR; ++r)
            if (u0 + r < U) g[(size_t)r * V] = (m.bad && u0 + r <= m.Lb) ? simple_nan() : 0.0f;
        return;
    }
    int ur[kSimpleR];
    bool mine[kSimpleR];
    float lmv[kSimpleR], acc[kSimpleR], occs[kSimpleR], ebs[kSimpleR], els[kSimpleR];
    const int *lab = p.labels + (size_t)b * (size_t)(U - 1);
#pragma unroll
    for (int r = 0; r < kSimpleR; ++r) {
        ur[r] = min(u0 + r, m.Lb);
        lmv[r] = p.lm[((size_t)b * U + ur[r]) * (size_t)V + v];
        mine[r] = ur[r] < m.Lb && min(max(lab[ur[r]], 0), V - 1) == v;
        acc[r] = occs[r] = ebs[r] = els[r] = 0.0f;
    }
    const float *amp = p.am + (size_t)b * T * (size_t)V + v;
    for (int t = 0; t < m.Tb; ++t) {
        const float amv = amp[(size_t)t * V];
#pragma unroll
        for (int r = 0; r < kSimpleR; ++r) {
            const size_t c = ((size_t)b * T + t) * (size_t)U + ur[r];
            const float2 e = p.e[c];
            const float occ = e.x + e.y;
            acc[r] += occ * __expf((amv + lmv[r]) - p.Z[c]);
            occs[r] += occ;
            ebs[r] += e.x;
            els[r] += e.y;
        }
    }
    const float cs = p.cost_scale ? p.cost_scale[b] : 1.0f;
#pragma unroll
    for (int r = 0; r < kSimpleR; ++r) {
        if (u0 + r >= U) break;
        const float sl = __expf(lmv[r] - p.Zl[(size_t)b * U + ur[r]]);
        const float eps = (v == p.blank ? ebs[r] : 0.0f) + (mine[r] ? els[r] : 0.0f);
        const float x = cs * (p.w_scale * acc[r] + p.l_scale * (sl * occs[r]) - (p.w_scale + p.l_scale) * eps);
        g[(size_t)r * V] = u0 + r <= m.Lb ? x : 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------
// Launchers.  Every grid is one-dimensional; the entry point has checked that its size fits.
// ---------------------------------------------------------------------------------------------
hipError_t launch_simple_rows(const SimpleParams &p, hipStream_t s) {
    const uint32_t rows = (uint32_t)p.B * (uint32_t)(p.T + p.U);
    hipLaunchKernelGGL(simple_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_simple_cells(const SimpleParams &p, hipStream_t s) {
    const int tiles_t = (p.T + kSimpleTile - 1) / kSimpleTile, tiles_u = (p.U + kSimpleTile - 1) / kSimpleTile;
    hipLaunchKernelGGL(simple_cells_kernel, dim3((uint32_t)p.B * tiles_t * tiles_u), dim3(256), 0, s, p, tiles_t, tiles_u);
    return hipGetLastError();
}

hipError_t launch_simple_occupancy(const SimpleParams &p, hipStream_t s) {
    const uint32_t ncells = (uint32_t)p.B * (uint32_t)p.T * (uint32_t)p.U;
    hipLaunchKernelGGL(simple_occupancy_kernel, dim3((ncells + 255) / 256), dim3(256), 0, s, p);
    return hipGetLastError();
}

int simple_grad_lanes(const int V) { return V <= 16 ? 16 : V <= 32 ? 32 : 64; }

template <int VL>
static hipError_t launch_simple_grads_VL(const SimpleParams &p, hipStream_t s) {
    constexpr int kRows = (256 / VL) * kSimpleR;
    const int nv = (p.V + VL - 1) / VL;
    const int nt = (p.T + kRows - 1) / kRows, nu = (p.U + kRows - 1) / kRows;
    hipLaunchKernelGGL((simple_grad_am_kernel<VL>), dim3((uint32_t)p.B * nv * nt), dim3(256), 0, s, p, nv, nt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((simple_grad_lm_kernel<VL>), dim3((uint32_t)p.B * nv * nu), dim3(256), 0, s, p, nv, nu);
    return hipGetLastError();
}

hipError_t launch_simple_grads(const SimpleParams &p, hipStream_t s) {
    switch (simple_grad_lanes(p.V)) {
        case 16: return launch_simple_grads_VL<16>(p, s);
        case 32: return launch_simple_grads_VL<32>(p, s);
        default: return launch_simple_grads_VL<64>(p, s);
    }
}

}  // namespace rnnt
