// lstm_train_kernels.hip -- one LSTM layer for TRAINING: a forward that keeps what the backward needs, and back-propagation
// through time (include/rnnt.h compute_rnnt_lstm_train_fwd / _bwd).
//
// R rows (the batch), T frames, hidden H, output width P (projected by a bias-free W_hr [P, H] when P < H; else P = H), torch's
// gate order i, f, g, o, zero initial state, no row lengths.  Every buffer is TIME-MAJOR: a frame's R rows are contiguous.
//   forward, t = 0 ... T-1           (the caller computed pre = x W_ih^T + b_ih + b_hh for every frame)
//     gates (lstm_train_step_kernel<LT_FWD_GATES>)  a = pre_t + r_{t-1} W_hh^T; the activated gates over pre_t in place; c_t; h_t
//     proj  (lstm_train_step_kernel<LT_FWD_PROJ>)   projected layers only: r_t = h_t W_hr^T into y[t]
//   backward, t = T-1 ... 0          (da over the gates in place)
//     dr    (lstm_train_step_kernel<LT_BWD_DR>)     projected layers only: dr_t = dy_t + da_{t+1} W_hh into dr[t]
//     cell  (lstm_train_step_kernel<LT_BWD_CELL>)   dh_t = dr_t W_hr (projected) or dy_t + da_{t+1} W_hh; then the cell: da_t
//                                                   over the gates of frame t, and dc_t f_t into the carry [R, H] for frame t - 1
// One launch per frame for an unprojected layer and two for a projected one, in each direction.  No launch waits for another
// workgroup: the frame-to-frame dependency is stream order, and no launch writes what another of its workgroups reads (the
// forward reads y[t-1] and writes frame t; the backward reads da[t+1] / dr[t] and writes da[t] / the carry element it owns).
//
// All four roles are one product, out[r, c] = sum_k x[r, k] W[k, c] for a tile of 32 columns and TR rows, with W packed k-major
// in the workspace once per call (lstm_train_pack_kernel, one launch per matrix):
//   forward gates  [r4(P)][4 r8(H)]  column 32 tile + 8 gate + u = unit 8 tile + u of that gate: a workgroup owns whole cells
//   forward proj   [r4(H)][r32(P)]   W_hr transposed
//   backward       W_hh [4H][r32(P)] and W_hr [r4(P)][r32(H)] as torch stores them (they are k-major for these products), padded
// Padding is zeros, so widths that are not multiples of the tiles are exact.  Every sum has an order fixed by the shapes alone:
// K is split into NKG interleaved groups of 4 (one FMA chain each, in k order; NKG depends on K only) and the NKG partials are
// added in group order.  The rows per workgroup only pick how many rows share a weight load, so a row's y, c, h, gates, da and
// dr are bitwise independent of the number of rows, of the other rows and of the call.
#include "../../include/rnnt.h"
#include "rnnt_common.h"

#include <math.h>

namespace rnnt {

constexpr int kLtMaxRows = 1024, kLtMaxWidth = 4096, kLtMaxFrames = 1 << 20;
constexpr int kLtLds = 150 * 1024;  // dynamic LDS budget of a step workgroup (160 KiB per CU)
constexpr int kLtMaxTr = 16;
constexpr int kLtFewWgs = 256;      // rows per workgroup are halved while the launch has fewer workgroups than CUs

static inline size_t lt_a64(size_t n) { return (n + 63) / 64 * 64; }
static inline int lt_r4(int n) { return (n + 3) / 4 * 4; }
static inline int lt_r8(int n) { return (n + 7) / 8 * 8; }
static inline int lt_r32(int n) { return (n + 31) / 32 * 32; }

struct LtLayout {
    int R, T, H, P;
    bool proj;
    int Hp;             // r8(H): the forward's gate tiles
    int Kp, Kh;         // r4(P), r4(H)
    int ldg, ldp, ldh;  // 4 Hp, r32(P), r32(H)
    // offsets in floats from the workspace base
    size_t whh_f, whr_f, whh_b, whr_b, carry, total;
};

static bool make_lt_layout(int R, int T, int H, int P, bool proj, LtLayout &o) {
    if (R < 1 || R > kLtMaxRows || T < 1 || T > kLtMaxFrames || H < 1 || H > kLtMaxWidth || P < 1 || P > H) return false;
    if (proj ? P >= H : P != H) return false;
    o.R = R, o.T = T, o.H = H, o.P = P, o.proj = proj;
    o.Hp = lt_r8(H), o.Kp = lt_r4(P), o.Kh = lt_r4(H);
    o.ldg = 4 * o.Hp, o.ldp = lt_r32(P), o.ldh = lt_r32(H);
    size_t off = 0;
    o.whh_f = off, off += lt_a64((size_t)o.Kp * o.ldg);
    o.whr_f = off, off += proj ? lt_a64((size_t)o.Kh * o.ldp) : 0;
    o.whh_b = off, off += lt_a64((size_t)4 * H * o.ldp);
    o.whr_b = off, off += proj ? lt_a64((size_t)o.Kp * o.ldh) : 0;
    o.carry = off, off += lt_a64((size_t)R * H);
    o.total = off;
    return true;
}

// ---------------------------------------------------------------------------------------------
// the weight images (once per call and matrix)
// ---------------------------------------------------------------------------------------------
// mode 0: LSTM gates, transposed.  src [4N][K] (torch rows i, f, g, o) -> dst [Kpad][ld], column c = 32 tile + 8 gate + u holds
//         unit 8 tile + u of that gate (0 past N).
// mode 1: transposed.  src [N][K] -> dst [Kpad][ld], column c = src row c (0 past N).
// mode 2: as stored.   src [K][N] -> dst [Kpad][ld] (0 past N and past K).
struct LtPack {
    float *dst;
    int Kpad, ld, mode;
    const float *src;
    int K, N;
};

__global__ __launch_bounds__(256) void lstm_train_pack_kernel(const LtPack p) {
    __shared__ float tile[64][65];  // [column - c0][k - k0]
    const int k0 = blockIdx.y * 64, c0 = blockIdx.x * 64, lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    if (p.mode == 2) {
        for (int i = ly; i < 64; i += 4) {
            const int k = k0 + i, c = c0 + lx;
            if (k < p.Kpad && c < p.ld) p.dst[(size_t)k * p.ld + c] = (k < p.K && c < p.N) ? p.src[(size_t)k * p.N + c] : 0.f;
        }
        return;
    }
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

// ---------------------------------------------------------------------------------------------
// the step of one frame
// ---------------------------------------------------------------------------------------------
enum { LT_FWD_GATES = 0, LT_FWD_PROJ = 1, LT_BWD_DR = 2, LT_BWD_CELL = 3 };

struct LtStep {
    const float *W;     // packed [Kpad][ld]
    int Kpad, ld, R;
    const float *x;     // the product's left side: x + r xs, K floats each; NULL: no product (the sum is 0)
    size_t xs;
    int K;
    int H, N;           // hidden width; the width of the launch's output (FWD_GATES and BWD_CELL: H; FWD_PROJ and BWD_DR: P)
    float *g;           // FWD_GATES: pre -> gates of this frame [R, 4H]; BWD_CELL: gates -> da
    const float *c;     // BWD_CELL: c of this frame [R, H]
    const float *cp;    // FWD_GATES / BWD_CELL: c of the frame before [R, H]; NULL at frame 0
    float *co;          // FWD_GATES: c of this frame
    const float *add;   // BWD_DR, and BWD_CELL of an unprojected layer: dy of this frame [R, N]; else NULL
    float *out;         // FWD_GATES: h (or y) [R, H]; FWD_PROJ: y [R, P]; BWD_DR: dr [R, P]
    float *carry;       // BWD_CELL: dc_{t+1} f_{t+1} in, dc_t f_t out [R, H]
    int last;           // BWD_CELL: frame T - 1 (the carry is not read)
};

__device__ __forceinline__ float lt_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// A workgroup owns 32 columns (8 quads) and TR rows; thread (g, q) = (tid >> 3, tid & 7) accumulates column quad q over the
// k quads g, g + NKG, ... in order (one FMA chain per (row, column)); the NKG partials are then added in group order.
template <int ROLE, int TR, int NKG>
__global__ __launch_bounds__(NKG * 8) void lstm_train_step_kernel(const LtStep a) {
    extern __shared__ float lt_sm[];
    float *xs = lt_sm;                  // [TR][Kpad]
    float *red = lt_sm + TR * a.Kpad;   // [NKG][TR][32]
    const int tid = threadIdx.x, q = tid & 7, g = tid >> 3;
    const int r0 = blockIdx.y * TR, c0 = blockIdx.x * 32;
    if (a.x) {
        for (int t = 0; t < TR; ++t) {
            const int r = r0 + t;
            const float *src = a.x + (size_t)r * a.xs;
            for (int k = tid; k < a.Kpad; k += NKG * 8) xs[t * a.Kpad + k] = (r < a.R && k < a.K) ? src[k] : 0.f;
        }
        __syncthreads();
    }

    float acc[TR][4];
#pragma unroll
    for (int t = 0; t < TR; ++t) acc[t][0] = acc[t][1] = acc[t][2] = acc[t][3] = 0.f;
    const int nq = a.x ? a.Kpad >> 2 : 0;
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

    if (ROLE == LT_FWD_GATES) {  // columns 8 gate + u of the tile: unit j = 8 tile + u
        for (int i = tid; i < TR * 8; i += NKG * 8) {
            const int t = i >> 3, u = i & 7, r = r0 + t, j = blockIdx.x * 8 + u;
            if (r >= a.R || j >= a.H) continue;
            const float *s = red + t * 32;
            float *p = a.g + (size_t)r * 4 * a.H + j;
            const size_t H = a.H, cell = (size_t)r * H + j;
            const float gi = lt_sigmoid(s[u] + p[0]), gf = lt_sigmoid(s[8 + u] + p[H]);
            const float gg = tanhf(s[16 + u] + p[2 * H]), go = lt_sigmoid(s[24 + u] + p[3 * H]);
            const float c = gf * (a.cp ? a.cp[cell] : 0.f) + gi * gg;
            p[0] = gi, p[H] = gf, p[2 * H] = gg, p[3 * H] = go;
            a.co[cell] = c;
            a.out[cell] = go * tanhf(c);
        }
    } else if (ROLE == LT_FWD_PROJ || ROLE == LT_BWD_DR) {
        for (int i = tid; i < TR * 32; i += NKG * 8) {
            const int t = i >> 5, n = c0 + (i & 31), r = r0 + t;
            if (r >= a.R || n >= a.N) continue;
            const size_t at = (size_t)r * a.N + n;
            a.out[at] = ROLE == LT_BWD_DR ? a.add[at] + red[i] : red[i];
        }
    } else {
        for (int i = tid; i < TR * 32; i += NKG * 8) {
            const int t = i >> 5, j = c0 + (i & 31), r = r0 + t;
            if (r >= a.R || j >= a.H) continue;
            const size_t H = a.H, cell = (size_t)r * H + j;
            const float dh = a.add ? a.add[cell] + red[i] : red[i];
            float *p = a.g + (size_t)r * 4 * H + j;
            const float gi = p[0], gf = p[H], gg = p[2 * H], go = p[3 * H];
            const float tc = tanhf(a.c[cell]), cprev = a.cp ? a.cp[cell] : 0.f;
            float dc = dh * go * (1.0f - tc * tc);
            if (!a.last) dc += a.carry[cell];
            p[0] = dc * gg * (gi * (1.0f - gi));
            p[H] = dc * cprev * (gf * (1.0f - gf));
            p[2 * H] = dc * gi * (1.0f - gg * gg);
            p[3 * H] = dh * tc * (go * (1.0f - go));
            a.carry[cell] = dc * gf;
        }
    }
}

// k groups: 32 (256 threads) up to K = 512, 64 (512 threads) beyond: the backward's K = 4H has four times the forward's length
static int lt_kgroups(int Kpad) { return Kpad > 512 ? 64 : 32; }

static int lt_rows_per_wg(int Kpad, int NKG, int R, int col_tiles) {
    int tr = kLtMaxTr;
    while (tr > 1 && (size_t)tr * (Kpad + NKG * 32) * sizeof(float) > (size_t)kLtLds) tr >>= 1;
    while (tr > 1 && tr / 2 >= R) tr >>= 1;
    while (tr > 1 && (long)col_tiles * ((R + tr - 1) / tr) < kLtFewWgs) tr >>= 1;
    return tr;
}

template <int ROLE, int TR, int NKG>
static hipError_t lt_launch_tr(const LtStep &a, dim3 grid, size_t shm, hipStream_t s) {
    const hipError_t e = set_lds(lstm_train_step_kernel<ROLE, TR, NKG>, shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((lstm_train_step_kernel<ROLE, TR, NKG>), grid, dim3(NKG * 8), shm, s, a);
    return hipGetLastError();
}

template <int ROLE, int NKG>
static hipError_t lt_launch_kg(const LtStep &a, hipStream_t s) {
    const int tr = lt_rows_per_wg(a.Kpad, NKG, a.R, a.ld / 32);
    const dim3 grid(a.ld / 32, (a.R + tr - 1) / tr);
    const size_t shm = (size_t)tr * (a.Kpad + NKG * 32) * sizeof(float);
    switch (tr) {
    case 16: return lt_launch_tr<ROLE, 16, NKG>(a, grid, shm, s);
    case 8: return lt_launch_tr<ROLE, 8, NKG>(a, grid, shm, s);
    case 4: return lt_launch_tr<ROLE, 4, NKG>(a, grid, shm, s);
    case 2: return lt_launch_tr<ROLE, 2, NKG>(a, grid, shm, s);
    default: return lt_launch_tr<ROLE, 1, NKG>(a, grid, shm, s);
    }
}

template <int ROLE>
static hipError_t lt_launch(const LtStep &a, hipStream_t s) {
    return lt_kgroups(a.Kpad) == 64 ? lt_launch_kg<ROLE, 64>(a, s) : lt_launch_kg<ROLE, 32>(a, s);
}

static hipError_t lt_pack(float *dst, int Kpad, int ld, int mode, const float *src, int K, int N, hipStream_t s) {
    LtPack p = {dst, Kpad, ld, mode, src, K, N};
    hipLaunchKernelGGL(lstm_train_pack_kernel, dim3((ld + 63) / 64, (Kpad + 63) / 64), dim3(256), 0, s, p);
    return hipGetLastError();
}

bool lstm_train_layout_ok(int R, int T, int H, int P, bool proj, size_t *bytes) {
    LtLayout o;
    if (!make_lt_layout(R, T, H, P, proj, o)) return false;
    if (bytes) *bytes = (o.total * sizeof(float) + 255) / 256 * 256;
    return true;
}

hipError_t launch_lstm_train_fwd(float *gates, const float *W_hh, const float *W_hr, float *y, float *c, float *h, int R, int T, int H,
                                 int P, void *workspace, hipStream_t s) {
    LtLayout o;
    if (!make_lt_layout(R, T, H, P, W_hr != nullptr, o)) return hipErrorInvalidValue;
    float *ws = (float *)workspace;
    hipError_t e;
    if ((e = lt_pack(ws + o.whh_f, o.Kp, o.ldg, 0, W_hh, P, H, s)) != hipSuccess) return e;
    if (o.proj && (e = lt_pack(ws + o.whr_f, o.Kh, o.ldp, 1, W_hr, H, P, s)) != hipSuccess) return e;
    const size_t fg = (size_t)R * 4 * H, fh = (size_t)R * H, fp = (size_t)R * P;
    for (int t = 0; t < T; ++t) {
        LtStep a = {};
        a.W = ws + o.whh_f, a.Kpad = o.Kp, a.ld = o.ldg, a.R = R;
        a.x = t ? y + (size_t)(t - 1) * fp : nullptr, a.xs = P, a.K = P;
        a.H = H, a.N = H;
        a.g = gates + (size_t)t * fg;
        a.cp = t ? c + (size_t)(t - 1) * fh : nullptr;
        a.co = c + (size_t)t * fh;
        a.out = o.proj ? h + (size_t)t * fh : y + (size_t)t * fh;
        if ((e = lt_launch<LT_FWD_GATES>(a, s)) != hipSuccess) return e;
        if (o.proj) {
            LtStep p = {};
            p.W = ws + o.whr_f, p.Kpad = o.Kh, p.ld = o.ldp, p.R = R;
            p.x = h + (size_t)t * fh, p.xs = H, p.K = H;
            p.H = H, p.N = P;
            p.out = y + (size_t)t * fp;
            if ((e = lt_launch<LT_FWD_PROJ>(p, s)) != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

hipError_t launch_lstm_train_bwd(float *gates, const float *c, const float *dy, const float *W_hh, const float *W_hr, float *dr, int R,
                                 int T, int H, int P, void *workspace, hipStream_t s) {
    LtLayout o;
    if (!make_lt_layout(R, T, H, P, W_hr != nullptr, o)) return hipErrorInvalidValue;
    float *ws = (float *)workspace;
    hipError_t e;
    if ((e = lt_pack(ws + o.whh_b, 4 * H, o.ldp, 2, W_hh, 4 * H, P, s)) != hipSuccess) return e;
    if (o.proj && (e = lt_pack(ws + o.whr_b, o.Kp, o.ldh, 2, W_hr, P, H, s)) != hipSuccess) return e;
    const size_t fg = (size_t)R * 4 * H, fh = (size_t)R * H, fp = (size_t)R * P;
    for (int t = T - 1; t >= 0; --t) {
        const float *da_next = t + 1 < T ? gates + (size_t)(t + 1) * fg : nullptr;
        LtStep a = {};
        a.R = R, a.H = H, a.N = H;
        if (o.proj) {
            LtStep d = {};
            d.W = ws + o.whh_b, d.Kpad = 4 * H, d.ld = o.ldp, d.R = R;
            d.x = da_next, d.xs = 4 * (size_t)H, d.K = 4 * H;
            d.H = H, d.N = P;
            d.add = dy + (size_t)t * fp;
            d.out = dr + (size_t)t * fp;
            if ((e = lt_launch<LT_BWD_DR>(d, s)) != hipSuccess) return e;
            a.W = ws + o.whr_b, a.Kpad = o.Kp, a.ld = o.ldh;
            a.x = dr + (size_t)t * fp, a.xs = P, a.K = P;
        } else {
            a.W = ws + o.whh_b, a.Kpad = 4 * H, a.ld = o.ldp;
            a.x = da_next, a.xs = 4 * (size_t)H, a.K = 4 * H;
            a.add = dy + (size_t)t * fp;
        }
        a.g = gates + (size_t)t * fg;
        a.c = c + (size_t)t * fh;
        a.cp = t ? c + (size_t)(t - 1) * fh : nullptr;
        a.carry = ws + o.carry;
        a.last = t == T - 1;
        if ((e = lt_launch<LT_BWD_CELL>(a, s)) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace rnnt
