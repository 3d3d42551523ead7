// encoder_kernels.hip -- the encoder's forward pass for every utterance of a batch (include/rnnt.h compute_rnnt_encoder_*).
//
// The network (model.py Encoder, eval mode): BatchNorm (running statistics) -> L blocks of {one-layer LSTM (optional
// projection) -> LayerNorm}, with TimeReduction (stack f frames, zero-pad the tail) after block `ridx`.  One run of T frames:
//   in      (enc_norm_kernel, mode 0)  X = BatchNorm(x) as a per-feature affine map: [R, T, F]
//   per block l, over its T_l frames (T_l = T up to block ridx, ceil(T / f) after it):
//     gemm  (enc_gemm_kernel)          pre = X W_ih^T + b_ih + b_hh for a window of frames of every row (the bulk of the FLOPs)
//     gates (enc_step_kernel<GATES>)   per frame: gates = pre_t + r_{t-1} W_hh^T, then the cell: c (in place), h
//     proj  (enc_step_kernel<PROJ>)    per frame, projected blocks only: r_t = h W_hr^T
//     norm  (enc_norm_kernel, mode 1)  X = LayerNorm_l(Y) -- stacked by f frames after block ridx, and the call's `out` after the
//                                      last block -- and the last frame's raw r into the state for the next run
// Y [R, T_l, P_l] holds the block's r for every frame: the gates launch of frame t reads r_{t-1} from Y (from the state at
// t = 0) and an unprojected block writes h straight to Y[t], so no launch overwrites what another workgroup of it reads.
// No launch waits for another workgroup: the frame-to-frame dependency is stream order.
//
// Weights are packed k-major in the workspace.  The gate columns come in tiles of 32: 8 hidden units x the 4 gates (i, f, g, o),
// so one workgroup of the step owns whole cells and H = 2048 gives 256 column tiles.  Every sum has a fixed order that depends
// on the shapes alone: the GEMM runs one FMA chain per output over k; the step kernel splits K into NKG interleaved groups of
// 4 (an FMA chain each, in k order) and adds the NKG partials in group order.  The rows per workgroup only pick how many rows
// share a weight load, so a row's results are bitwise independent of the number of rows, of the other rows and of the run.
#include "../../include/rnnt.h"
#include "rnnt_common.h"

#include <math.h>

namespace rnnt {

constexpr int kEnMaxRows = 1024, kEnMaxLayers = 16, kEnMaxWidth = 4096, kEnMaxFactor = 16;
constexpr int kEnLds = 150 * 1024;                  // dynamic LDS budget of a step workgroup (160 KiB per CU)
constexpr size_t kEnPreBytes = (size_t)64 << 20;    // the input-GEMM window: at most this many bytes of `pre` (or one frame)

static inline size_t a64(size_t n) { return (n + 63) / 64 * 64; }
static inline int r4(int n) { return (n + 3) / 4 * 4; }
static inline int r8(int n) { return (n + 7) / 8 * 8; }

struct EnLayout {
    int R, L, F, ridx, f, Tmax;
    int H[kEnMaxLayers], P[kEnMaxLayers], In[kEnMaxLayers], Hp[kEnMaxLayers];
    int Ki[kEnMaxLayers], Kh[kEnMaxLayers], Kr[kEnMaxLayers], ldr[kEnMaxLayers];
    bool proj[kEnMaxLayers];
    float eps[kEnMaxLayers], bn_eps;
    // offsets in floats from the workspace base
    size_t r[kEnMaxLayers], c[kEnMaxLayers];  // the state (first in the workspace)
    size_t hbuf, X, Y, pre, Xn, Yn, pren;
    size_t bn_mean, bn_scale, bn_bias;
    size_t wi[kEnMaxLayers], wh[kEnMaxLayers], b[kEnMaxLayers], wr[kEnMaxLayers], lng[kEnMaxLayers], lnb[kEnMaxLayers];
    size_t total;
};

static int frames_of(const EnLayout &o, int l, int T) { return l > o.ridx ? (T + o.f - 1) / o.f : T; }

// frames per input-GEMM window of block l
static int window_of(const EnLayout &o, int l, int Tl) {
    const size_t per = (size_t)o.R * 4 * o.Hp[l] * sizeof(float);
    size_t w = kEnPreBytes / per;
    if (w < 1) w = 1;
    return (int)(w < (size_t)Tl ? w : (size_t)Tl);
}

static bool make_en_layout(const rnntPrednetBlock *blocks, int L, int F, const float bn_eps, int ridx, int f, int R, int Tmax,
                           EnLayout &o) {
    if (!blocks || L < 1 || L > kEnMaxLayers || F < 1 || F > kEnMaxWidth || R < 1 || R > kEnMaxRows) return false;
    if (ridx < 0 || ridx >= L - 1 || f < 1 || f > kEnMaxFactor || Tmax < 1 || Tmax > (1 << 20)) return false;
    if (!(bn_eps >= 0.f)) return false;
    o.R = R, o.L = L, o.F = F, o.ridx = ridx, o.f = f, o.Tmax = Tmax, o.bn_eps = bn_eps;
    size_t off = 0, hmax = 0, xn = (size_t)Tmax * F, yn = 0, pren = 0;
    for (int l = 0; l < L; ++l) {
        const rnntPrednetBlock &b = blocks[l];
        if (b.hidden < 1 || b.hidden > kEnMaxWidth || b.proj < 1 || b.proj > kEnMaxWidth) return false;
        if (!b.W_hr && b.proj != b.hidden) return false;
        if (!(b.ln_eps >= 0.f)) return false;
        o.H[l] = b.hidden, o.P[l] = b.proj, o.proj[l] = b.W_hr != nullptr, o.eps[l] = b.ln_eps;
        o.In[l] = l == 0 ? F : (l == ridx + 1 ? f * o.P[l - 1] : o.P[l - 1]);
        if (o.In[l] > kEnMaxWidth) return false;
        o.Hp[l] = r8(o.H[l]);
        o.Ki[l] = r4(o.In[l]);
        o.Kh[l] = r4(o.P[l]);
        o.Kr[l] = r4(o.H[l]);
        o.ldr[l] = (int)a64(o.P[l]);
        const int Tl = frames_of(o, l, Tmax);
        const size_t xl = (size_t)Tl * o.In[l], yl = (size_t)Tl * o.P[l];
        if (xl > xn) xn = xl;
        if (yl > yn) yn = yl;
        if (o.proj[l] && (size_t)o.H[l] > hmax) hmax = o.H[l];
        const size_t pl = (size_t)window_of(o, l, Tl) * R * 4 * o.Hp[l];
        if (pl > pren) pren = pl;
        o.r[l] = off, off += a64((size_t)R * o.P[l]);
        o.c[l] = off, off += a64((size_t)R * o.H[l]);
    }
    // the last block's LayerNorm goes to `out`; the stacked input of block ridx + 1 is no larger than Y's frames x f
    o.Xn = a64(xn * R), o.Yn = a64(yn * R), o.pren = a64(pren);
    o.hbuf = off, off += a64((size_t)R * hmax);
    o.X = off, off += o.Xn;
    o.Y = off, off += o.Yn;
    o.pre = off, off += o.pren;
    o.bn_mean = off, off += a64(F);
    o.bn_scale = off, off += a64(F);
    o.bn_bias = off, off += a64(F);
    for (int l = 0; l < L; ++l) {
        const size_t ng = 4 * (size_t)o.Hp[l];
        o.wi[l] = off, off += a64((size_t)o.Ki[l] * ng);
        o.wh[l] = off, off += a64((size_t)o.Kh[l] * ng);
        o.b[l] = off, off += a64(ng);
        o.wr[l] = off, off += o.proj[l] ? (size_t)o.Kr[l] * o.ldr[l] : 0;
        o.lng[l] = off, off += a64(o.P[l]);
        o.lnb[l] = off, off += a64(o.P[l]);
    }
    o.total = off;
    return true;
}

// ---------------------------------------------------------------------------------------------
// begin: the weight image
// ---------------------------------------------------------------------------------------------
// mode 0: LSTM gates.  src [4N][K] (torch rows i, f, g, o) -> dst [Kpad][4 Np], column c = 32 tile + 8 gate + u holds unit
//         8 tile + u of that gate (0 past N).
// mode 1: projection.  src [N][K] -> dst [Kpad][ld], column c = src row c (0 past N).
struct EnPack {
    float *dst;
    int Kpad, ld, mode;
    const float *src;
    int K, N;
};

__global__ __launch_bounds__(256) void encoder_pack_kernel(const EnPack p) {
    __shared__ float tile[64][65];  // [column - c0][k - k0]
    const int k0 = blockIdx.y * 64, c0 = blockIdx.x * 64, lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (int i = ly; i < 64; i += 4) {  // column c0 + i, k = k0 + lx: a source row read along k
        const int c = c0 + i, k = k0 + lx;
        int row = -1;
        if (p.mode == 0) {
            const int j = (c >> 5) * 8 + (c & 7);
            if (c < p.ld && j < p.N) row = ((c >> 3) & 3) * p.N + j;
        } else if (c < p.N) {
            row = c;
        }
        tile[i][lx] = (row >= 0 && k < p.K) ? p.src[(size_t)row * p.K + k] : 0.f;
    }
    __syncthreads();
    for (int i = ly; i < 64; i += 4) {
        const int k = k0 + i, c = c0 + lx;
        if (k < p.Kpad && c < p.ld) p.dst[(size_t)k * p.ld + c] = tile[lx][i];
    }
}

// mode 0: b_ih + b_hh in packed gate-column order (n = 4 Np columns); mode 1: the BatchNorm's mean, scale = weight /
// sqrt(var + eps) and bias (n = F); mode 2: plain copies of two vectors (the LayerNorm's gamma and beta)
__global__ __launch_bounds__(256) void encoder_vec_kernel(float *d0, float *d1, float *d2, const float *s0, const float *s1,
                                                          const float *s2, const float *s3, int N, int n, float eps, int mode) {
    for (int c = blockIdx.x * 256 + threadIdx.x; c < n; c += gridDim.x * 256) {
        if (mode == 2) {
            d0[c] = s0[c];
            d1[c] = s1[c];
            continue;
        }
        if (mode == 1) {
            d0[c] = s0[c];
            d1[c] = s2[c] / sqrtf(s1[c] + eps);
            d2[c] = s3[c];
            continue;
        }
        const int j = (c >> 5) * 8 + (c & 7), row = ((c >> 3) & 3) * N + j;
        d0[c] = j < N ? s0[row] + s1[row] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------
// run: BatchNorm in / LayerNorm out
// ---------------------------------------------------------------------------------------------
// ragged rows (compute_rnnt_encoder_run_rows): the frames row r has at a block whose frames are its input's reduced by div
__device__ __forceinline__ int en_row_frames(const int *rf, const int r, const int div) {
    return (max(rf[r], 0) + div - 1) / div;
}

__device__ __forceinline__ float en_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return __shfl(v, 0, 64);
}

struct EnNorm {
    const float *src;  // mode 0: x [R, T, W]; mode 1: Y [R, T, W]
    float *dst;        // [R, ceil(T / f), f W]: frame t of row r at (r ceil(T / f) + t / f) f W + (t % f) W
    float *state;      // mode 1: the raw last frame of every row -> [R, W]
    const float *g, *b, *m;  // mode 0: scale, bias, mean; mode 1: gamma, beta
    float eps;
    int R, T, W, f, mode;
    const int *rf;     // mode 1: row_frames of a ragged run (frames of row r: en_row_frames(rf, r, div)), or NULL: T each
    int div;
};

// one wave per (row, frame) of the padded frame range; frames past T are written as zeros
__global__ __launch_bounds__(256) void enc_norm_kernel(const EnNorm a) {
    const int lane = threadIdx.x & 63;
    const int Tq = (a.T + a.f - 1) / a.f, Tp = Tq * a.f;
    const long idx = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= (long)a.R * Tp) return;
    const int r = (int)(idx / Tp), t = (int)(idx % Tp);
    float *d = a.dst + ((size_t)r * Tq + t / a.f) * ((size_t)a.f * a.W) + (size_t)(t % a.f) * a.W;
    const int Tr = (a.mode == 1 && a.rf) ? min(en_row_frames(a.rf, r, a.div), a.T) : a.T;  // the row's frames (its last: the state)
    if (t >= Tr) {
        for (int k = lane; k < a.W; k += 64) d[k] = 0.f;
        return;
    }
    const float *s = a.src + ((size_t)r * a.T + t) * a.W;
    if (a.mode == 0) {
        for (int k = lane; k < a.W; k += 64) d[k] = fmaf(s[k] - a.m[k], a.g[k], a.b[k]);
        return;
    }
    float sum = 0.f;
    for (int k = lane; k < a.W; k += 64) sum += s[k];
    const float mean = en_wave_sum(sum) / (float)a.W;
    float q = 0.f;
    for (int k = lane; k < a.W; k += 64) {
        const float dv = s[k] - mean;
        q = fmaf(dv, dv, q);
    }
    const float rstd = 1.0f / sqrtf(en_wave_sum(q) / (float)a.W + a.eps);
    for (int k = lane; k < a.W; k += 64) d[k] = fmaf((s[k] - mean) * rstd, a.g[k], a.b[k]);
    if (t == Tr - 1)
        for (int k = lane; k < a.W; k += 64) a.state[(size_t)r * a.W + k] = s[k];
}

// ---------------------------------------------------------------------------------------------
// run: the input GEMM  pre[m, c] = sum_k X[m, k] Wp[k, c] + bias[c],  m = r Wn + (t - t0)
// ---------------------------------------------------------------------------------------------
struct EnGemm {
    const float *X;     // [R, Tl, K]
    const float *W;     // packed [Kpad][ld]
    const float *bias;  // [ld]
    float *pre;         // [R Wn][ld]
    int K, Kpad, ld, Tl, t0, Wn, M;
};

constexpr int kGmTile = 128, kGmKc = 8;

// 256 threads, a 128 x 128 tile, 8 x 8 outputs per thread (rows ty*4 + {0..3} and 64 + ty*4 + {0..3}, columns likewise by tx);
// every output is one FMA chain over k = 0 ... K-1 in order.
__global__ __launch_bounds__(256) void enc_gemm_kernel(const EnGemm a) {
    __shared__ float As[kGmKc][kGmTile + 4];
    __shared__ float Bs[kGmKc][kGmTile];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.y * kGmTile, n0 = blockIdx.x * kGmTile;
    // A loader: row m0 + (tid >> 1), k = kk + (tid & 1) * 4 + {0..3}
    const int am = m0 + (tid >> 1), ak = (tid & 1) * 4;
    const float *arow = nullptr;
    if (am < a.M) {
        const int r = am / a.Wn, t = a.t0 + am % a.Wn;
        arow = a.X + ((size_t)r * a.Tl + t) * a.K;
    }
    // B loader: k = kk + (tid >> 5), columns n0 + (tid & 31) * 4 + {0..3}
    const int bk = tid >> 5, bn = n0 + (tid & 31) * 4;
    float acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    for (int kk = 0; kk < a.Kpad; kk += kGmKc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = kk + ak + i;
            As[ak + i][tid >> 1] = (arow && k < a.K) ? arow[k] : 0.f;
        }
        {
            const int k = kk + bk;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < a.Kpad && bn < a.ld) v = *reinterpret_cast<const float4 *>(a.W + (size_t)k * a.ld + bn);
            *reinterpret_cast<float4 *>(&Bs[bk][(tid & 31) * 4]) = v;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kGmKc; ++k) {
            const float4 a0 = *reinterpret_cast<const float4 *>(&As[k][ty * 4]);
            const float4 a1 = *reinterpret_cast<const float4 *>(&As[k][64 + ty * 4]);
            const float4 b0 = *reinterpret_cast<const float4 *>(&Bs[k][tx * 4]);
            const float4 b1 = *reinterpret_cast<const float4 *>(&Bs[k][64 + tx * 4]);
            const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int m = m0 + (i < 4 ? ty * 4 + i : 64 + ty * 4 + i - 4);
        if (m >= a.M) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = n0 + h * 64 + tx * 4;
            if (n >= a.ld) continue;
            const float4 bb = *reinterpret_cast<const float4 *>(a.bias + n);
            float4 v;
            v.x = acc[i][h * 4 + 0] + bb.x;
            v.y = acc[i][h * 4 + 1] + bb.y;
            v.z = acc[i][h * 4 + 2] + bb.z;
            v.w = acc[i][h * 4 + 3] + bb.w;
            *reinterpret_cast<float4 *>(a.pre + (size_t)m * a.ld + n) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// run: the recurrent step (gates + cell, or the projection) for one frame
// ---------------------------------------------------------------------------------------------
enum { EN_GATES = 0, EN_PROJ = 1 };

struct EnStep {
    const float *W;      // packed [Kpad][ld]
    int Kpad, ld, R;
    const float *x;      // staged rows: x + r xs, K floats each (zero past K)
    size_t xs;
    int K;
    // gates
    const float *pre;    // pre + r ps: the row's 4 Np gate pre-activations of this frame
    size_t ps;
    float *c;            // [R, N] in place
    // both: out + r os (gates: h [.., N]; proj: r [.., N])
    float *out;
    size_t os;
    int N;
    // ragged run: rows with frame t >= en_row_frames(rf, r, div) neither write nor update c (rf NULL: every row runs)
    const int *rf;
    int t, div;
};

__device__ __forceinline__ float en_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// A workgroup owns 32 columns (8 quads) and TR rows; thread (g, q) = (tid >> 3, tid & 7) accumulates column quad q over the
// k quads g, g + NKG, ... in order (one FMA chain per (row, column)); the NKG partials are then added in group order.
template <int ROLE, int TR, int NKG>
__global__ __launch_bounds__(NKG * 8) void enc_step_kernel(const EnStep a) {
    extern __shared__ float en_sm[];
    float *xs = en_sm;                  // [TR][Kpad]
    float *red = en_sm + TR * a.Kpad;   // [NKG][TR][32]
    const int tid = threadIdx.x, q = tid & 7, g = tid >> 3;
    const int r0 = blockIdx.y * TR, c0 = blockIdx.x * 32;
    for (int t = 0; t < TR; ++t) {
        const int r = r0 + t;
        const float *src = a.x + (size_t)r * a.xs;
        for (int k = tid; k < a.Kpad; k += NKG * 8) xs[t * a.Kpad + k] = (r < a.R && k < a.K) ? src[k] : 0.f;
    }
    __syncthreads();

    float acc[TR][4];
#pragma unroll
    for (int t = 0; t < TR; ++t) acc[t][0] = acc[t][1] = acc[t][2] = acc[t][3] = 0.f;
    const int nq = a.Kpad >> 2;
    const size_t ld = a.ld;
    const float *w = a.W + c0 + 4 * q;
#pragma unroll 2
    for (int kq = g; kq < nq; kq += NKG) {
        const float *wk = w + (size_t)(4 * kq) * ld;
        const float4 w0 = *reinterpret_cast<const float4 *>(wk);
        const float4 w1 = *reinterpret_cast<const float4 *>(wk + ld);
        const float4 w2 = *reinterpret_cast<const float4 *>(wk + 2 * ld);
        const float4 w3 = *reinterpret_cast<const float4 *>(wk + 3 * ld);
#pragma unroll
        for (int t = 0; t < TR; ++t) {
            const float4 xv = *reinterpret_cast<const float4 *>(xs + t * a.Kpad + 4 * kq);
            acc[t][0] = fmaf(xv.x, w0.x, acc[t][0]);
            acc[t][1] = fmaf(xv.x, w0.y, acc[t][1]);
            acc[t][2] = fmaf(xv.x, w0.z, acc[t][2]);
            acc[t][3] = fmaf(xv.x, w0.w, acc[t][3]);
            acc[t][0] = fmaf(xv.y, w1.x, acc[t][0]);
            acc[t][1] = fmaf(xv.y, w1.y, acc[t][1]);
            acc[t][2] = fmaf(xv.y, w1.z, acc[t][2]);
            acc[t][3] = fmaf(xv.y, w1.w, acc[t][3]);
            acc[t][0] = fmaf(xv.z, w2.x, acc[t][0]);
            acc[t][1] = fmaf(xv.z, w2.y, acc[t][1]);
            acc[t][2] = fmaf(xv.z, w2.z, acc[t][2]);
            acc[t][3] = fmaf(xv.z, w2.w, acc[t][3]);
            acc[t][0] = fmaf(xv.w, w3.x, acc[t][0]);
            acc[t][1] = fmaf(xv.w, w3.y, acc[t][1]);
            acc[t][2] = fmaf(xv.w, w3.z, acc[t][2]);
            acc[t][3] = fmaf(xv.w, w3.w, acc[t][3]);
        }
    }
#pragma unroll
    for (int t = 0; t < TR; ++t)
        *reinterpret_cast<float4 *>(red + ((size_t)g * TR + t) * 32 + 4 * q) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    __syncthreads();
    for (int i = tid; i < TR * 8; i += NKG * 8) {  // the partials in group order: quad i of row i / 8 -> group 0's slot
        float4 s = *reinterpret_cast<const float4 *>(red + 4 * i);
        for (int v = 1; v < NKG; ++v) {
            const float4 p = *reinterpret_cast<const float4 *>(red + (size_t)v * TR * 32 + 4 * i);
            s.x += p.x, s.y += p.y, s.z += p.z, s.w += p.w;
        }
        *reinterpret_cast<float4 *>(red + 4 * i) = s;
    }
    __syncthreads();

    if (ROLE == EN_GATES) {
        for (int i = tid; i < TR * 8; i += NKG * 8) {
            const int t = i >> 3, u = i & 7, r = r0 + t, j = blockIdx.x * 8 + u;
            if (r >= a.R || j >= a.N) continue;
            if (a.rf && a.t >= en_row_frames(a.rf, r, a.div)) continue;
            const float *s = red + t * 32, *p = a.pre + (size_t)r * a.ps + c0;
            const float gi = s[u] + p[u], gf = s[8 + u] + p[8 + u], gg = s[16 + u] + p[16 + u], go = s[24 + u] + p[24 + u];
            float *cp = a.c + (size_t)r * a.N + j;
            const float c = en_sigmoid(gf) * *cp + en_sigmoid(gi) * tanhf(gg);
            *cp = c;
            a.out[(size_t)r * a.os + j] = en_sigmoid(go) * tanhf(c);
        }
    } else {
        for (int i = tid; i < TR * 32; i += NKG * 8) {
            const int t = i >> 5, n = c0 + (i & 31), r = r0 + t;
            if (r >= a.R || n >= a.N) continue;
            if (a.rf && a.t >= en_row_frames(a.rf, r, a.div)) continue;
            a.out[(size_t)r * a.os + n] = red[i];
        }
    }
}

// Threads per step workgroup: the gates launch has 4 Np / 32 column tiles (256 at H = 2048) and takes 32 k groups; the
// projection has only P / 32 (20 at P = 640) and a longer K, so it takes 64 k groups: more weight loads in flight per CU.
constexpr int kEnGatesKg = 32, kEnProjKg = 64, kEnMaxTr = 16;

static int en_rows_per_wg(int Kpad, int NKG, int R) {
    int tr = kEnMaxTr;
    while (tr > 1 && (size_t)tr * (Kpad + NKG * 32) * sizeof(float) > (size_t)kEnLds) tr >>= 1;
    while (tr > 1 && tr / 2 >= R) tr >>= 1;
    return tr;
}

template <int ROLE, int TR, int NKG>
static hipError_t en_launch_tr(const EnStep &a, dim3 grid, size_t shm, hipStream_t s) {
    const hipError_t e = set_lds(enc_step_kernel<ROLE, TR, NKG>, shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((enc_step_kernel<ROLE, TR, NKG>), grid, dim3(NKG * 8), shm, s, a);
    return hipGetLastError();
}

template <int ROLE, int NKG>
static hipError_t en_launch(const EnStep &a, hipStream_t s) {
    const int tr = en_rows_per_wg(a.Kpad, NKG, a.R);
    const dim3 grid(a.ld / 32, (a.R + tr - 1) / tr);
    const size_t shm = (size_t)tr * (a.Kpad + NKG * 32) * sizeof(float);
    switch (tr) {
    case 16: return en_launch_tr<ROLE, 16, NKG>(a, grid, shm, s);
    case 8: return en_launch_tr<ROLE, 8, NKG>(a, grid, shm, s);
    case 4: return en_launch_tr<ROLE, 4, NKG>(a, grid, shm, s);
    case 2: return en_launch_tr<ROLE, 2, NKG>(a, grid, shm, s);
    default: return en_launch_tr<ROLE, 1, NKG>(a, grid, shm, s);
    }
}

static hipError_t en_norm(const EnNorm &n, hipStream_t s) {
    const long rows = (long)n.R * ((n.T + n.f - 1) / n.f) * n.f;
    hipLaunchKernelGGL(enc_norm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, n);
    return hipGetLastError();
}

// ragged run: zero the state (r and c of every block) of the rows with reset[r] != 0; blockIdx.y = 2 l + (0: r, 1: c)
struct EnReset {
    float *base[2 * kEnMaxLayers];
    int W[2 * kEnMaxLayers];
    const int *reset;
    int R;
};

__global__ __launch_bounds__(256) void enc_reset_kernel(const EnReset a) {
    float *p = a.base[blockIdx.y];
    const int W = a.W[blockIdx.y];
    const size_t n = (size_t)a.R * W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        if (a.reset[i / W] != 0) p[i] = 0.f;
}

static hipError_t en_run(const EnLayout &o, float *ws, const float *x, int T, float *out, const int *rf, const int *reset,
                         hipStream_t s) {
    hipError_t e;
    const int R = o.R;
    if (reset) {
        EnReset z = {};
        size_t n = 0;
        for (int l = 0; l < o.L; ++l) {
            z.base[2 * l] = ws + o.r[l], z.W[2 * l] = o.P[l];
            z.base[2 * l + 1] = ws + o.c[l], z.W[2 * l + 1] = o.H[l];
            n = (size_t)R * (o.P[l] > o.H[l] ? o.P[l] : o.H[l]) > n ? (size_t)R * (o.P[l] > o.H[l] ? o.P[l] : o.H[l]) : n;
        }
        z.reset = reset, z.R = R;
        const size_t g = (n + 255) / 256;
        hipLaunchKernelGGL(enc_reset_kernel, dim3((unsigned)(g < 1024 ? g : 1024), 2 * o.L), dim3(256), 0, s, z);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    {  // BatchNorm into X
        EnNorm n = {};
        n.src = x, n.dst = ws + o.X, n.g = ws + o.bn_scale, n.b = ws + o.bn_bias, n.m = ws + o.bn_mean;
        n.R = R, n.T = T, n.W = o.F, n.f = 1, n.mode = 0;
        if ((e = en_norm(n, s)) != hipSuccess) return e;
    }
    for (int l = 0; l < o.L; ++l) {
        const int Tl = frames_of(o, l, T), Wn = window_of(o, l, Tl), ld = 4 * o.Hp[l];
        float *Y = ws + o.Y;
        for (int t0 = 0; t0 < Tl; t0 += Wn) {
            const int wn = Tl - t0 < Wn ? Tl - t0 : Wn;
            EnGemm gm = {ws + o.X, ws + o.wi[l], ws + o.b[l], ws + o.pre, o.In[l], o.Ki[l], ld, Tl, t0, wn, R * wn};
            hipLaunchKernelGGL(enc_gemm_kernel, dim3((ld + kGmTile - 1) / kGmTile, (gm.M + kGmTile - 1) / kGmTile), dim3(256), 0, s,
                               gm);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            for (int t = t0; t < t0 + wn; ++t) {
                EnStep a = {};
                a.W = ws + o.wh[l], a.Kpad = o.Kh[l], a.ld = ld, a.R = R;
                if (t == 0) a.x = ws + o.r[l], a.xs = o.P[l];
                else a.x = Y + (size_t)(t - 1) * o.P[l], a.xs = (size_t)Tl * o.P[l];
                a.K = o.P[l];
                a.pre = ws + o.pre + (size_t)(t - t0) * ld, a.ps = (size_t)wn * ld;
                a.c = ws + o.c[l], a.N = o.H[l];
                a.rf = rf, a.t = t, a.div = l > o.ridx ? o.f : 1;
                if (o.proj[l]) a.out = ws + o.hbuf, a.os = o.H[l];
                else a.out = Y + (size_t)t * o.P[l], a.os = (size_t)Tl * o.P[l];
                if ((e = en_launch<EN_GATES, kEnGatesKg>(a, s)) != hipSuccess) return e;
                if (o.proj[l]) {
                    EnStep p = {};
                    p.W = ws + o.wr[l], p.Kpad = o.Kr[l], p.ld = o.ldr[l], p.R = R;
                    p.x = ws + o.hbuf, p.xs = o.H[l], p.K = o.H[l];
                    p.out = Y + (size_t)t * o.P[l], p.os = (size_t)Tl * o.P[l], p.N = o.P[l];
                    p.rf = rf, p.t = t, p.div = a.div;
                    if ((e = en_launch<EN_PROJ, kEnProjKg>(p, s)) != hipSuccess) return e;
                }
            }
        }
        EnNorm n = {};  // LayerNorm of Y into the next block's input (stacked after ridx) or `out`; the last r into the state
        n.src = Y, n.dst = l + 1 < o.L ? ws + o.X : out, n.state = ws + o.r[l];
        n.g = ws + o.lng[l], n.b = ws + o.lnb[l], n.eps = o.eps[l];
        n.R = R, n.T = Tl, n.W = o.P[l], n.f = l == o.ridx ? o.f : 1, n.mode = 1;
        n.rf = rf, n.div = l > o.ridx ? o.f : 1;
        if ((e = en_norm(n, s)) != hipSuccess) return e;
    }
    return hipSuccess;
}

static hipError_t en_pack(float *dst, int Kpad, int ld, int mode, const float *src, int K, int N, hipStream_t s) {
    EnPack p = {dst, Kpad, ld, mode, src, K, N};
    hipLaunchKernelGGL(encoder_pack_kernel, dim3((ld + 63) / 64, (Kpad + 63) / 64), dim3(256), 0, s, p);
    return hipGetLastError();
}

static hipError_t en_vec(float *d0, float *d1, float *d2, const float *s0, const float *s1, const float *s2, const float *s3, int N,
                         int n, float eps, int mode, hipStream_t s) {
    const int g = (n + 255) / 256;
    hipLaunchKernelGGL(encoder_vec_kernel, dim3(g < 1024 ? g : 1024), dim3(256), 0, s, d0, d1, d2, s0, s1, s2, s3, N, n, eps, mode);
    return hipGetLastError();
}

bool encoder_layout_ok(const rnntPrednetBlock *blocks, int L, int F, float bn_eps, int ridx, int f, int R, int Tmax, size_t *bytes) {
    EnLayout o;
    if (!make_en_layout(blocks, L, F, bn_eps, ridx, f, R, Tmax, o)) return false;
    if (bytes) *bytes = o.total * sizeof(float);
    return true;
}

hipError_t launch_encoder_begin(const rnntPrednetBlock *blocks, int L, int F, const float *bn_mean, const float *bn_var,
                                const float *bn_weight, const float *bn_bias, float bn_eps, int ridx, int f, int R, int Tmax,
                                void *workspace, hipStream_t s) {
    EnLayout o;
    if (!make_en_layout(blocks, L, F, bn_eps, ridx, f, R, Tmax, o)) return hipErrorInvalidValue;
    float *ws = (float *)workspace;
    hipError_t e;
    if ((e = en_vec(ws + o.bn_mean, ws + o.bn_scale, ws + o.bn_bias, bn_mean, bn_var, bn_weight, bn_bias, 0, F, bn_eps, 1, s)) !=
        hipSuccess)
        return e;
    for (int l = 0; l < L; ++l) {
        const rnntPrednetBlock &b = blocks[l];
        const int ng = 4 * o.Hp[l];
        if ((e = en_pack(ws + o.wi[l], o.Ki[l], ng, 0, b.W_ih, o.In[l], o.H[l], s)) != hipSuccess) return e;
        if ((e = en_pack(ws + o.wh[l], o.Kh[l], ng, 0, b.W_hh, o.P[l], o.H[l], s)) != hipSuccess) return e;
        if ((e = en_vec(ws + o.b[l], nullptr, nullptr, b.b_ih, b.b_hh, nullptr, nullptr, o.H[l], ng, 0.f, 0, s)) != hipSuccess) return e;
        if (o.proj[l] && (e = en_pack(ws + o.wr[l], o.Kr[l], o.ldr[l], 1, b.W_hr, o.H[l], o.P[l], s)) != hipSuccess) return e;
        if ((e = en_vec(ws + o.lng[l], ws + o.lnb[l], nullptr, b.ln_weight, b.ln_bias, nullptr, nullptr, 0, o.P[l], 0.f, 2, s)) !=
            hipSuccess)
            return e;
    }
    return launch_fill(ws, 0, o.hbuf * sizeof(float), s);  // every row's state (r, c) = 0
}

hipError_t launch_encoder_run(const float *x, int T, float *out, const rnntPrednetBlock *blocks, int L, int F, float bn_eps, int ridx,
                              int f, int R, int Tmax, void *workspace, hipStream_t s) {
    EnLayout o;
    if (!make_en_layout(blocks, L, F, bn_eps, ridx, f, R, Tmax, o) || T < 1 || T > Tmax) return hipErrorInvalidValue;
    return en_run(o, (float *)workspace, x, T, out, nullptr, nullptr, s);
}

hipError_t launch_encoder_run_rows(const float *x, int T, const int *row_frames, const int *reset, float *out,
                                   const rnntPrednetBlock *blocks, int L, int F, float bn_eps, int ridx, int f, int R, int Tmax,
                                   void *workspace, hipStream_t s) {
    EnLayout o;
    if (!make_en_layout(blocks, L, F, bn_eps, ridx, f, R, Tmax, o) || T < 1 || T > Tmax || !row_frames) return hipErrorInvalidValue;
    return en_run(o, (float *)workspace, x, T, out, row_frames, reset, s);
}

}  // namespace rnnt
