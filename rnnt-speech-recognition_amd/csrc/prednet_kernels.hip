// prednet_kernels.hip -- one prediction-network step for every decoder row (include/rnnt.h compute_rnnt_prednet_*).
//
// The network (model.py PredictionNetwork, inference): embedding -> L blocks of {one-layer LSTM (optional projection) ->
// LayerNorm} -> the joint's first Dense layer without its bias (pred_proj = x W1).  One step, per block l:
//   gates   (prednet_kernel<PN_GATES>)  gates = [x, r_prev] [W_ih; W_hh]^T + b_ih + b_hh for a tile of 16 hidden units (all four
//           gates: 64 packed columns) and a tile of TR rows, then the cell: c, h.  x is staged in LDS: block 0 the embedding row of
//           the row's token, block l > 0 the LayerNorm of block l-1's new r, applied on load (every workgroup normalises the rows
//           it stages itself: no extra launch, no cross-workgroup hand-off).  An unprojected block writes h as its new r.
//   proj    (prednet_kernel<PN_PROJ>)   r = h W_hr^T (projected blocks only).
//   out     (prednet_kernel<PN_OUT>)    pred_proj = LayerNorm_{L-1}(r) W1, applied on load as above.
// L = 2 projected blocks: 5 launches per step, none of them waits for another workgroup.
//
// All three are one GEMM body: out[r, n] = sum_k x[r, k] W[k, n] over a packed k-major weight image (columns padded to 64 with
// zeros, rows to a multiple of 4).  A workgroup owns 64 columns (one per lane) and TR rows; its NW waves split K into NW fixed
// contiguous ranges, each wave accumulates its range in k order with one f32 FMA chain per (row, column), and the NW partials are
// added in wave order.  The split depends on K alone and TR only picks how many rows share a weight load, so every result is
// bitwise independent of the number of rows, of the other rows and of the run.
//
// State: r and c of every block and pred_proj, double-buffered by step parity (ctl[0] = the slot holding the current state).
// A step reads slot cur and writes slot cur ^ 1, so a beam step may gather any row; the last workgroup of the out launch to
// finish (an atomic count, no waiting) flips ctl[0] for the next step.
#include "../../include/rnnt.h"
#include "rnnt_common.h"

#include <math.h>

namespace rnnt {

constexpr int kPnMaxRows = 1024, kPnMaxBlocks = 8, kPnMaxWidth = 4096;
constexpr int kPnLds = 150 * 1024;  // dynamic LDS budget of a GEMM workgroup (the staged rows + the partial sums; 160 KiB per CU)

enum { PN_GATES = 0, PN_PROJ = 1, PN_OUT = 2 };

static inline size_t a64(size_t n) { return (n + 63) / 64 * 64; }
static inline int r4(int n) { return (n + 3) / 4 * 4; }

struct PnLayout {
    int R, L, E, V, Jp;
    int H[kPnMaxBlocks], P[kPnMaxBlocks], In[kPnMaxBlocks], Hpad[kPnMaxBlocks], Kg[kPnMaxBlocks], Kp[kPnMaxBlocks];
    bool proj[kPnMaxBlocks];
    float eps[kPnMaxBlocks];
    // offsets in floats from the workspace base
    size_t S;                                   // slot stride of the state region
    size_t r[kPnMaxBlocks], c[kPnMaxBlocks];    // slot-0 state of block l
    size_t pp, ppS;                             // pred_proj slots and their stride
    size_t ctl, hbuf;
    size_t emb, wg[kPnMaxBlocks], bi[kPnMaxBlocks], bh[kPnMaxBlocks], wr[kPnMaxBlocks], lng[kPnMaxBlocks], lnb[kPnMaxBlocks], w1;
    int Kw1;
    size_t total;  // floats
};

static bool make_pn_layout(const rnntPrednetBlock *blocks, int L, int E, int V, int Jp, int R, PnLayout &o) {
    if (!blocks || L < 1 || L > kPnMaxBlocks || E < 1 || E > kPnMaxWidth || V < 1 || R < 1 || R > kPnMaxRows) return false;
    if (Jp < 64 || Jp > 704 || Jp % 64 != 0) return false;
    o.R = R, o.L = L, o.E = E, o.V = V, o.Jp = Jp;
    size_t off = 0, hmax = 0;
    for (int l = 0; l < L; ++l) {
        const rnntPrednetBlock &b = blocks[l];
        if (b.hidden < 1 || b.hidden > kPnMaxWidth || b.proj < 1 || b.proj > kPnMaxWidth) return false;
        if (!b.W_hr && b.proj != b.hidden) return false;
        if (!(b.ln_eps >= 0.f)) return false;
        o.H[l] = b.hidden, o.P[l] = b.proj, o.proj[l] = b.W_hr != nullptr, o.eps[l] = b.ln_eps;
        o.In[l] = l == 0 ? E : o.P[l - 1];
        o.Hpad[l] = (b.hidden + 15) / 16 * 16;
        o.Kg[l] = r4(o.In[l] + o.P[l]);
        o.Kp[l] = r4(o.H[l]);
        o.r[l] = off, off += a64((size_t)R * o.P[l]);
        o.c[l] = off, off += a64((size_t)R * o.H[l]);
        if (o.proj[l] && (size_t)o.H[l] > hmax) hmax = o.H[l];
    }
    o.S = off;
    off *= 2;
    o.ppS = a64((size_t)R * Jp);
    o.pp = off, off += 2 * o.ppS;
    o.ctl = off, off += 64;
    o.hbuf = off, off += a64((size_t)R * hmax);
    o.emb = off, off += a64((size_t)V * E);
    for (int l = 0; l < L; ++l) {
        const size_t ng = 4 * (size_t)o.Hpad[l];
        o.wg[l] = off, off += a64((size_t)o.Kg[l] * ng);
        o.bi[l] = off, off += a64(ng);
        o.bh[l] = off, off += a64(ng);
        o.wr[l] = off, off += o.proj[l] ? a64((size_t)o.Kp[l] * a64(o.P[l])) : 0;
        o.lng[l] = off, off += a64(o.P[l]);
        o.lnb[l] = off, off += a64(o.P[l]);
    }
    o.Kw1 = r4(o.P[L - 1]);
    o.w1 = off, off += a64((size_t)o.Kw1 * Jp);
    o.total = off;
    return true;
}

// ---------------------------------------------------------------------------------------------
// begin: the weight image
// ---------------------------------------------------------------------------------------------
struct PnPack {
    float *dst;       // [Kpad][ld]
    int Kpad, ld;
    int mode;         // 0: LSTM gates (W_ih | W_hh, 16 units x 4 gates per 64 columns); 1: src [N][K] transposed; 2: src [K][N]
    const float *s0, *s1;
    int K0, K1, N;    // mode 0: K0 = in, K1 = proj, N = hidden; modes 1 / 2: K0 = K, N = columns
};

__global__ __launch_bounds__(256) void prednet_pack_kernel(const PnPack p) {
    __shared__ float tile[64][65];  // [k - k0][column - c0]
    const int k0 = blockIdx.y * 64, c0 = blockIdx.x * 64, lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (int i = ly; i < 64; i += 4) {
        float v = 0.f;
        if (p.mode == 2) {  // row k0 + i of a k-major source, column c0 + lx
            const int k = k0 + i, c = c0 + lx;
            if (k < p.K0 && c < p.N) v = p.s0[(size_t)k * p.N + c];
            tile[i][lx] = v;
        } else {  // column c0 + i, k = k0 + lx: a source row read along k
            const int c = c0 + i, k = k0 + lx;
            if (p.mode == 1) {
                if (c < p.N && k < p.K0) v = p.s0[(size_t)c * p.K0 + k];
            } else {
                const int cc = c & 63, j = (c >> 6) * 16 + (cc & 15), row = (cc >> 4) * p.N + j;
                if (j < p.N) {
                    if (k < p.K0) v = p.s0[(size_t)row * p.K0 + k];
                    else if (k < p.K0 + p.K1) v = p.s1[(size_t)row * p.K1 + (k - p.K0)];
                }
            }
            tile[lx][i] = v;
        }
    }
    __syncthreads();
    for (int i = ly; i < 64; i += 4) {
        const int k = k0 + i;
        if (k < p.Kpad) p.dst[(size_t)k * p.ld + c0 + lx] = tile[i][lx];
    }
}

// gate biases in packed column order (0 for padding units); mode 1: a plain copy of n floats
__global__ __launch_bounds__(256) void prednet_vec_kernel(float *bi, float *bh, const float *si, const float *sh, int H, int n,
                                                          int mode) {
    for (int c = blockIdx.x * 256 + threadIdx.x; c < n; c += gridDim.x * 256) {
        if (mode == 1) {
            bi[c] = si[c];
            continue;
        }
        const int cc = c & 63, j = (c >> 6) * 16 + (cc & 15), row = (cc >> 4) * H + j;
        bi[c] = j < H ? si[row] : 0.f;
        bh[c] = j < H ? sh[row] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------
// step: the GEMM body with its three prologues / epilogues
// ---------------------------------------------------------------------------------------------
struct PnArgs {
    const float *W;               // packed [Kpad][ld]
    const float *bias_i, *bias_h; // gates: [ld] packed order
    int Kpad, ld, R, N;           // N: gates: hidden units; proj / out: real columns
    const int *emitted;           // NULL: token 0 for every row (begin)
    const int *parents;           // NULL: src = r
    const int *reset;             // compute_rnnt_prednet_reset (emitted, parents NULL): reset[r] != 0 runs token 0 from zero
                                  // state, the other rows carry over
    int *ctl;                     // [0] slot of the current state, [1] finished workgroups of the out launch
    size_t S;                     // state slot stride (floats)
    // staged x = [segment A (width A), segment B (width Bw)]
    int mode_a;                   // 0: embedding row of tok; 1: LayerNorm of a row of the NEW slot; 2: raw row (hbuf)
    const float *a_base;          // mode 0: embedding [V, A]; 1: slot-0 r of the previous block; 2: hbuf
    int A;
    const float *ln_g, *ln_b;
    float eps;
    const float *b_base;          // slot-0 r of this block (row src of the CURRENT slot), or NULL
    int Bw;
    // outputs
    float *c_base;                // gates: slot-0 c [R, N]
    float *h_out;                 // gates: slot-0 r [R, N] (unprojected) or hbuf [R, N]
    int h_state;                  // 1: h_out is the r state (slot stride S)
    float *o_base;                // proj: slot-0 r [R, N]; out: pred_proj slot 0 [R, N]
    size_t oS;                    // its slot stride
    float *out2;                  // out: pred_proj_out
};

__device__ __forceinline__ float pn_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// the sum of a wave, lane 0's value broadcast (a fixed tree: every lane, every wave, every run gets the same bits)
__device__ __forceinline__ float pn_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return __shfl(v, 0, 64);
}

template <int ROLE, int TR, int NW>
__global__ __launch_bounds__(NW * 64) void prednet_kernel(const PnArgs a) {
    extern __shared__ float pn_sm[];
    float *xs = pn_sm;                 // [TR][Kpad]
    float *red = pn_sm + TR * a.Kpad;  // [NW][TR][64]
    __shared__ int s_tok[TR], s_src[TR], s_zero[TR], s_cur;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r0 = blockIdx.y * TR;
    if (tid < TR) {
        const int r = r0 + tid;
        int tok = -1, src = 0, zero = 0;  // rows beyond R: staged as zeros, never stored
        if (r < a.R) {
            tok = a.emitted ? a.emitted[r] : 0;
            src = a.parents ? min(max(a.parents[r], 0), a.R - 1) : r;
            if (a.reset) zero = a.reset[r] != 0, tok = zero ? 0 : -1;
        }
        s_tok[tid] = tok, s_src[tid] = src, s_zero[tid] = zero;
    }
    if (tid == 0) s_cur = __hip_atomic_load(a.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1;
    __syncthreads();
    const int cur = s_cur, nxt = cur ^ 1;

    // ---- stage the TR input rows
    for (int t = 0; t < TR; ++t) {
        const int r = r0 + t, tok = s_tok[t], src = s_src[t];
        const bool live = r < a.R;
        float *x = xs + t * a.Kpad;
        for (int k = tid; k < a.A; k += NW * 64) {
            float v = 0.f;
            if (a.mode_a == 0) {
                if (tok >= 0) v = a.a_base[(size_t)tok * a.A + k];
            } else if (live) {
                v = a.a_base[(a.mode_a == 1 ? nxt * a.S : 0) + (size_t)r * a.A + k];
            }
            x[k] = v;
        }
        for (int k = tid; k < a.Bw; k += NW * 64) x[a.A + k] = (live && !s_zero[t]) ? a.b_base[cur * a.S + (size_t)src * a.Bw + k] : 0.f;
        for (int k = a.A + a.Bw + tid; k < a.Kpad; k += NW * 64) x[k] = 0.f;
    }
    __syncthreads();
    if (a.mode_a == 1) {  // LayerNorm of segment A, one wave per row (biased variance, two passes)
        for (int t = wv; t < TR; t += NW) {
            float *x = xs + t * a.Kpad;
            float s = 0.f;
            for (int k = lane; k < a.A; k += 64) s += x[k];
            const float mean = pn_wave_sum(s) / (float)a.A;
            float q = 0.f;
            for (int k = lane; k < a.A; k += 64) {
                const float d = x[k] - mean;
                q = fmaf(d, d, q);
            }
            const float rstd = 1.0f / sqrtf(pn_wave_sum(q) / (float)a.A + a.eps);
            for (int k = lane; k < a.A; k += 64) x[k] = fmaf((x[k] - mean) * rstd, a.ln_g[k], a.ln_b[k]);
        }
        __syncthreads();
    }

    // ---- this wave's K range, one FMA chain per (row, column) in k order
    const int col = blockIdx.x * 64 + lane;
    const int kc = ((a.Kpad / 4 + NW - 1) / NW) * 4;
    const int k0 = min(wv * kc, a.Kpad), k1 = min(k0 + kc, a.Kpad);
    float acc[TR];
#pragma unroll
    for (int t = 0; t < TR; ++t) acc[t] = 0.f;
    const size_t ld = a.ld;
    const float *w = a.W + (size_t)k0 * ld + col;
#pragma unroll 4
    for (int k = k0; k < k1; k += 4, w += 4 * ld) {
        const float w0 = w[0], w1 = w[ld], w2 = w[2 * ld], w3 = w[3 * ld];
#pragma unroll
        for (int t = 0; t < TR; ++t) {
            const float4 xv = *reinterpret_cast<const float4 *>(xs + t * a.Kpad + k);
            acc[t] = fmaf(xv.x, w0, acc[t]);
            acc[t] = fmaf(xv.y, w1, acc[t]);
            acc[t] = fmaf(xv.z, w2, acc[t]);
            acc[t] = fmaf(xv.w, w3, acc[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < TR; ++t) red[(wv * TR + t) * 64 + lane] = acc[t];
    __syncthreads();
    for (int i = tid; i < TR * 64; i += NW * 64) {  // the partials in wave order
        float s = red[i];
        for (int v = 1; v < NW; ++v) s += red[v * TR * 64 + i];
        red[i] = s;
    }
    __syncthreads();

    // ---- epilogues
    if (ROLE == PN_GATES) {
        for (int i = tid; i < TR * 16; i += NW * 64) {
            const int t = i >> 4, u = i & 15, j = blockIdx.x * 16 + u, r = r0 + t;
            if (r >= a.R || j >= a.N) continue;
            const int tok = s_tok[t], src = s_src[t];
            float *cn = a.c_base + nxt * a.S + (size_t)r * a.N + j;
            const float cp = s_zero[t] ? 0.f : a.c_base[cur * a.S + (size_t)src * a.N + j];
            float *hn = a.h_out + (a.h_state ? nxt * a.S : 0) + (size_t)r * a.N + j;
            if (tok < 0) {
                *cn = cp;
                *hn = a.h_state ? a.h_out[cur * a.S + (size_t)src * a.N + j] : 0.f;
                continue;
            }
            const float *g = red + t * 64;
            const int cb = blockIdx.x * 64 + u;
            const float gi = g[u] + a.bias_i[cb] + a.bias_h[cb];
            const float gf = g[16 + u] + a.bias_i[cb + 16] + a.bias_h[cb + 16];
            const float gg = g[32 + u] + a.bias_i[cb + 32] + a.bias_h[cb + 32];
            const float go = g[48 + u] + a.bias_i[cb + 48] + a.bias_h[cb + 48];
            const float c = pn_sigmoid(gf) * cp + pn_sigmoid(gi) * tanhf(gg);
            *cn = c;
            *hn = pn_sigmoid(go) * tanhf(c);
        }
    } else {
        for (int i = tid; i < TR * 64; i += NW * 64) {
            const int t = i >> 6, n = blockIdx.x * 64 + (i & 63), r = r0 + t;
            if (r >= a.R || n >= a.N) continue;
            const float v = s_tok[t] < 0 ? a.o_base[cur * a.oS + (size_t)s_src[t] * a.N + n] : red[i];
            a.o_base[nxt * a.oS + (size_t)r * a.N + n] = v;
            if (ROLE == PN_OUT) a.out2[(size_t)r * a.N + n] = v;
        }
    }
    if (ROLE == PN_OUT) {  // the last workgroup to finish moves the current slot on (every workgroup read ctl[0] above)
        __syncthreads();
        if (tid == 0) {
            __threadfence();
            const unsigned nblk = gridDim.x * gridDim.y;
            if (atomicAdd((unsigned *)&a.ctl[1], 1u) == nblk - 1) {
                atomicExch(&a.ctl[1], 0);
                atomicExch(&a.ctl[0], nxt);
            }
        }
    }
}

// rows per workgroup: as many as the LDS budget holds (at most max_tr), no more than the rows there are
static int pn_rows_per_wg(int Kpad, int NW, int R, int max_tr) {
    int tr = max_tr;
    while (tr > 1 && (size_t)tr * (Kpad + NW * 64) * sizeof(float) > (size_t)kPnLds) tr >>= 1;
    while (tr > 1 && tr / 2 >= R) tr >>= 1;
    return tr;
}

template <int ROLE, int TR, int NW>
static hipError_t pn_launch_tr(const PnArgs &a, dim3 grid, size_t shm, hipStream_t s) {
    const hipError_t e = set_lds(prednet_kernel<ROLE, TR, NW>, shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((prednet_kernel<ROLE, TR, NW>), grid, dim3(NW * 64), shm, s, a);
    return hipGetLastError();
}

template <int ROLE, int NW>
static hipError_t pn_launch(const PnArgs &a, int col_tiles, int max_tr, hipStream_t s) {
    const int tr = pn_rows_per_wg(a.Kpad, NW, a.R, max_tr);
    const dim3 grid(col_tiles, (a.R + tr - 1) / tr);
    const size_t shm = (size_t)tr * (a.Kpad + NW * 64) * sizeof(float);
    switch (tr) {
    case 16: return pn_launch_tr<ROLE, 16, NW>(a, grid, shm, s);
    case 8: return pn_launch_tr<ROLE, 8, NW>(a, grid, shm, s);
    case 4: return pn_launch_tr<ROLE, 4, NW>(a, grid, shm, s);
    case 2: return pn_launch_tr<ROLE, 2, NW>(a, grid, shm, s);
    default: return pn_launch_tr<ROLE, 1, NW>(a, grid, shm, s);
    }
}

// Waves per workgroup (the K split) and rows per workgroup at most.  The gates launch has 4 H / 64 column tiles; the projection
// and W1 launches have only P / 64 and Jp / 64 (10 at the reference defaults), so they take more waves and fewer rows per
// workgroup: more weight loads in flight per CU, more workgroups.
constexpr int kPnGatesWaves = 8, kPnDenseWaves = 16, kPnGatesRows = 16, kPnDenseRows = 4;

static hipError_t pn_step(const PnLayout &o, float *ws, const int *emitted, const int *parents, float *out, hipStream_t s,
                          const int *reset = nullptr) {
    hipError_t e;
    for (int l = 0; l < o.L; ++l) {
        PnArgs a = {};
        a.emitted = emitted, a.parents = parents, a.reset = reset, a.ctl = (int *)(ws + o.ctl), a.S = o.S, a.R = o.R;
        a.W = ws + o.wg[l], a.bias_i = ws + o.bi[l], a.bias_h = ws + o.bh[l];
        a.Kpad = o.Kg[l], a.ld = 4 * o.Hpad[l], a.N = o.H[l];
        if (l == 0) {
            a.mode_a = 0, a.a_base = ws + o.emb, a.A = o.E;
        } else {
            a.mode_a = 1, a.a_base = ws + o.r[l - 1], a.A = o.P[l - 1];
            a.ln_g = ws + o.lng[l - 1], a.ln_b = ws + o.lnb[l - 1], a.eps = o.eps[l - 1];
        }
        a.b_base = ws + o.r[l], a.Bw = o.P[l];
        a.c_base = ws + o.c[l];
        a.h_state = o.proj[l] ? 0 : 1;
        a.h_out = o.proj[l] ? ws + o.hbuf : ws + o.r[l];
        if ((e = pn_launch<PN_GATES, kPnGatesWaves>(a, o.Hpad[l] / 16, kPnGatesRows, s)) != hipSuccess) return e;
        if (o.proj[l]) {
            PnArgs p = {};
            p.emitted = emitted, p.parents = parents, p.reset = reset, p.ctl = (int *)(ws + o.ctl), p.S = o.S, p.R = o.R;
            p.W = ws + o.wr[l], p.Kpad = o.Kp[l], p.ld = (int)a64(o.P[l]), p.N = o.P[l];
            p.mode_a = 2, p.a_base = ws + o.hbuf, p.A = o.H[l];
            p.o_base = ws + o.r[l], p.oS = o.S;
            if ((e = pn_launch<PN_PROJ, kPnDenseWaves>(p, p.ld / 64, kPnDenseRows, s)) != hipSuccess) return e;
        }
    }
    const int l = o.L - 1;
    PnArgs q = {};
    q.emitted = emitted, q.parents = parents, q.reset = reset, q.ctl = (int *)(ws + o.ctl), q.S = o.S, q.R = o.R;
    q.W = ws + o.w1, q.Kpad = o.Kw1, q.ld = o.Jp, q.N = o.Jp;
    q.mode_a = 1, q.a_base = ws + o.r[l], q.A = o.P[l];
    q.ln_g = ws + o.lng[l], q.ln_b = ws + o.lnb[l], q.eps = o.eps[l];
    q.o_base = ws + o.pp, q.oS = o.ppS, q.out2 = out;
    return pn_launch<PN_OUT, kPnDenseWaves>(q, o.Jp / 64, kPnDenseRows, s);
}

static hipError_t pn_pack(float *dst, int Kpad, int ld, int mode, const float *s0, const float *s1, int K0, int K1, int N,
                          hipStream_t s) {
    PnPack p = {dst, Kpad, ld, mode, s0, s1, K0, K1, N};
    hipLaunchKernelGGL(prednet_pack_kernel, dim3(ld / 64, (Kpad + 63) / 64), dim3(256), 0, s, p);
    return hipGetLastError();
}

static hipError_t pn_copy(float *dst, const float *src, size_t n, hipStream_t s) {
    const size_t g = (n + 255) / 256;
    hipLaunchKernelGGL(prednet_vec_kernel, dim3((unsigned)(g < 2048 ? g : 2048)), dim3(256), 0, s, dst, nullptr, src, nullptr, 0,
                       (int)n, 1);
    return hipGetLastError();
}

bool prednet_layout_ok(const rnntPrednetBlock *blocks, int L, int E, int V, int Jp, int R, size_t *bytes) {
    PnLayout o;
    if (!make_pn_layout(blocks, L, E, V, Jp, R, o)) return false;
    if ((size_t)V * E > 0x7fffffffu) return false;  // (the copy kernel counts in int)
    if (bytes) *bytes = o.total * sizeof(float);
    return true;
}

hipError_t launch_prednet_begin(const float *emb, const rnntPrednetBlock *blocks, int L, int E, int V, const float *W1, int Jp, int R,
                                float *out, void *workspace, hipStream_t s) {
    PnLayout o;
    if (!make_pn_layout(blocks, L, E, V, Jp, R, o)) return hipErrorInvalidValue;
    float *ws = (float *)workspace;
    hipError_t e;
    if ((e = pn_copy(ws + o.emb, emb, (size_t)V * E, s)) != hipSuccess) return e;
    for (int l = 0; l < L; ++l) {
        const rnntPrednetBlock &b = blocks[l];
        const int ng = 4 * o.Hpad[l];
        if ((e = pn_pack(ws + o.wg[l], o.Kg[l], ng, 0, b.W_ih, b.W_hh, o.In[l], o.P[l], o.H[l], s)) != hipSuccess) return e;
        hipLaunchKernelGGL(prednet_vec_kernel, dim3((ng + 255) / 256), dim3(256), 0, s, ws + o.bi[l], ws + o.bh[l], b.b_ih, b.b_hh,
                           o.H[l], ng, 0);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (o.proj[l] && (e = pn_pack(ws + o.wr[l], o.Kp[l], (int)a64(o.P[l]), 1, b.W_hr, nullptr, o.H[l], 0, o.P[l], s)) != hipSuccess)
            return e;
        if ((e = pn_copy(ws + o.lng[l], b.ln_weight, o.P[l], s)) != hipSuccess) return e;
        if ((e = pn_copy(ws + o.lnb[l], b.ln_bias, o.P[l], s)) != hipSuccess) return e;
    }
    if ((e = pn_pack(ws + o.w1, o.Kw1, Jp, 2, W1, nullptr, o.P[L - 1], 0, Jp, s)) != hipSuccess) return e;
    // zero state in both slots, pred_proj slots, ctl = {0, 0}
    if ((e = launch_fill(ws, 0, (o.ctl + 64) * sizeof(float), s)) != hipSuccess) return e;
    return pn_step(o, ws, nullptr, nullptr, out, s);
}

hipError_t launch_prednet_step(const int *emitted, const int *parents, float *out, const rnntPrednetBlock *blocks, int L, int E,
                               int V, int Jp, int R, void *workspace, hipStream_t s) {
    PnLayout o;
    if (!make_pn_layout(blocks, L, E, V, Jp, R, o)) return hipErrorInvalidValue;
    return pn_step(o, (float *)workspace, emitted, parents, out, s);
}

// one step in which the rows with reset[r] != 0 run the start token 0 from zero state (what begin runs for every row) and the
// other rows carry their state and pred_proj over; it moves the parity slot on like any step
hipError_t launch_prednet_reset(const int *reset, float *out, const rnntPrednetBlock *blocks, int L, int E, int V, int Jp, int R,
                                void *workspace, hipStream_t s) {
    PnLayout o;
    if (!make_pn_layout(blocks, L, E, V, Jp, R, o) || !reset) return hipErrorInvalidValue;
    return pn_step(o, (float *)workspace, nullptr, nullptr, out, s, reset);
}

}  // namespace rnnt
