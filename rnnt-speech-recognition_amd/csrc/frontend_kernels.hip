// frontend_kernels.hip -- the streaming log-mel front end (include/rnnt.h, STREAMING FRONT END): raw audio chunks in, stacked
// log-mel rows out, for a batch of slots, the state kept in the workspace.
//
// A feed is two launches:
//   fe_frames_kernel  grid (frame tiles, slots), 4 waves.  One wave64 per STFT frame, the frames of a tile spread over the waves:
//                     gather carry ++ chunk, window, radix-2 decimation-in-frequency FFT in the wave's own LDS region (natural
//                     order in, bit-reversed out), magnitude, mel band sum (a lane per filter, ascending bin order), log.  Writes
//                     the raw log-mel frame x to the workspace; reads the carry, never writes it.
//   fe_emit_kernel    grid (slots), a thread per mel bin.  Scans the slot's new frames in stream order (running mean), stacks
//                     held ++ new frames into rows, zero-fills the rows past the count, keeps the frames that do not fill a group,
//                     and -- after a barrier behind which every read of the old carry lies -- writes the new carry and the state.
// The carry is rewritten by the second launch only: stream order puts that after every wave of the first has read it.
//
// LDS of fe_frames_kernel<N>: per wave re[N] + im[N] + mag[N/2 + 1] floats, plus the twiddles of every stage ([N] float2, the
// stage of half-span h at h ... 2h-1, so each stage reads consecutive words): 24 KB at N = 512 (six workgroups per CU), 96 KB at N = 2048 (one).  In a stage
// of half-span h < 32 the 32 lanes of an LDS group touch every second h-block of 64 consecutive words: 2-way bank conflicts,
// none from h = 32 up; the bit-reversed magnitude read is N/64-way (one read pass of N/2 + 1 words per frame).
//
// Every sum has an order fixed by the shapes alone (the butterflies of a frame, the band sum k = lo ... hi, the running sum in
// frame order): a frame's x and y are bitwise independent of the chunking, the slot, the slot count and the other slots.
#include "../../include/rnnt.h"
#include "rnnt_common.h"

#include <math.h>

namespace rnnt {

struct FeArgs {
    // tables and state (workspace)
    const float *window;  // [L]
    const float *wt;      // [M, nbp]: the mel matrix transposed, a filter's weights contiguous
    const int *blo, *bhi; // [M]: filter j sums the bins blo[j] ... bhi[j]-1
    const float2 *tw;     // [N]: stage of half-span h at h ... 2h-1: exp(-2 pi i j / 2h)
    int *st_c, *st_n, *st_h, *st_fin;  // [S] each
    float *msum;          // [S, M]
    float *carry;         // [S, L]
    float *held;          // [S, G, M]
    float *x;             // [S, NF, M]
    // the call
    const float *audio;   // [S, cs]
    const int *samples, *reset, *final_;
    float *rows;          // [S, max_rows, M * stack]
    int *counts;          // [S]
    int cs, norm;
    int S, L, step, M, stack, rm, G, logN, nbp, NF, max_rows;
};

struct FePack {
    const float *window_in, *mel_in;  // [L], [nb, M]
    float *window, *wt;
    int *blo, *bhi;
    float2 *tw;
    int *state;   // [4, S]
    float *zero;  // msum ... held, contiguous
    size_t zero_n;
    int S, L, M, N, nb, nbp;
};

namespace {

constexpr int kFeWaves = 4;         // waves of fe_frames_kernel
constexpr int kFeTile = 16;         // frames of one workgroup (four per wave)
constexpr int kFeEmitThreads = 128;
constexpr int kFeMaxLen = 2048;     // frame_len and nfft

struct FeLayout {
    int K, S, L, step, M, stack, rm, G, N, logN, nb, nbp, NF, max_rows;
    size_t window, wt, blo, bhi, tw, state, msum, carry, held, x, bytes;  // byte offsets
};

inline size_t a256(size_t n) { return (n + 255) / 256 * 256; }

bool make_fe_layout(int K, int S, int L, int step, int M, int stack, int rm, FeLayout *o) {
    if (K < 1 || K > (1 << 20) || S < 1 || S > 1024 || L < 2 || L > kFeMaxLen || step < 1 || step > L) return false;
    if (M < 1 || M > 1024 || stack < 1 || stack > 16 || rm < 1 || rm > 16) return false;
    int N = 1, logN = 0;
    while (N < L) N *= 2, ++logN;
    if (N < 256 || N > kFeMaxLen) return false;
    FeLayout l{};
    l.K = K, l.S = S, l.L = L, l.step = step, l.M = M, l.stack = stack, l.rm = rm, l.G = stack * rm, l.N = N, l.logN = logN;
    l.nb = N / 2 + 1;
    l.nbp = (l.nb + 3) / 4 * 4;
    l.NF = 1 + (K - 1) / step;  // frames one feed can complete: avail <= L - 1 + K
    l.max_rows = (l.G - 1 + l.NF) / stack;
    if ((long long)S * l.max_rows * M * stack >= (1ll << 31) || (long long)S * l.NF * M >= (1ll << 31)) return false;
    size_t off = 0;
    l.window = off, off += a256(sizeof(float) * L);
    l.wt = off, off += a256(sizeof(float) * (size_t)M * l.nbp);
    l.blo = off, off += a256(sizeof(int) * M);
    l.bhi = off, off += a256(sizeof(int) * M);
    l.tw = off, off += a256(sizeof(float2) * N);
    l.state = off, off += a256(sizeof(int) * 4 * (size_t)S);
    l.msum = off, off += a256(sizeof(float) * (size_t)S * M);
    l.carry = off, off += a256(sizeof(float) * (size_t)S * L);
    l.held = off, off += a256(sizeof(float) * (size_t)S * l.G * M);
    l.x = off, off += a256(sizeof(float) * (size_t)S * l.NF * M);
    l.bytes = off;
    *o = l;
    return true;
}

// what a slot does in this call, from its state and the call's arguments (the same in both kernels)
struct FeSlot {
    int c, k, nf, live, fin, rst;
};

__device__ inline FeSlot fe_slot(const FeArgs &a, int s) {
    FeSlot o;
    o.rst = a.reset ? (a.reset[s] != 0) : 0;
    o.live = o.rst || a.st_fin[s] == 0;
    o.c = o.rst ? 0 : min(max(a.st_c[s], 0), a.L - 1);
    o.k = o.live ? min(max(a.samples[s], 0), a.cs) : 0;
    o.fin = o.live && a.final_ && a.final_[s] != 0;
    const int avail = o.c + o.k;
    o.nf = (!o.live || avail < a.L) ? 0 : 1 + (avail - a.L) / a.step;
    return o;
}

// LDS accesses of one wave to its own region: program order is execution order; this keeps the compiler from moving them
__device__ inline void fe_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace

__global__ __launch_bounds__(256) void fe_pack_kernel(const FePack p) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
    for (size_t i = tid; i < (size_t)p.L; i += nth) p.window[i] = p.window_in[i];
    for (size_t i = tid; i < (size_t)p.M * p.nbp; i += nth) {
        const int j = (int)(i / p.nbp), k = (int)(i % p.nbp);
        p.wt[i] = k < p.nb ? p.mel_in[(size_t)k * p.M + j] : 0.f;
    }
    for (size_t j = tid; j < (size_t)p.M; j += nth) {  // the band of filter j: first ... last non-zero weight
        int lo = p.nb, hi = 0;
        for (int k = 0; k < p.nb; ++k)
            if (p.mel_in[(size_t)k * p.M + j] != 0.f) lo = min(lo, k), hi = k + 1;
        p.blo[j] = hi ? lo : 0, p.bhi[j] = hi;
    }
    for (size_t i = tid; i < (size_t)p.N; i += nth) {  // float64, rounded once
        float2 w = make_float2(1.f, 0.f);
        if (i >= 1) {
            int h = 1;
            while (2 * h <= (int)i) h *= 2;
            const double t = (double)((int)i - h) / (double)h;  // angle / pi = 2 j / 2h
            w = make_float2((float)cospi(t), (float)(-sinpi(t)));
        }
        p.tw[i] = w;
    }
    for (size_t i = tid; i < (size_t)4 * p.S; i += nth) p.state[i] = i >= (size_t)3 * p.S ? 1 : 0;  // every slot FINISHED
    for (size_t i = tid; i < p.zero_n; i += nth) p.zero[i] = 0.f;
}

template <int N>
__global__ __launch_bounds__(kFeWaves * 64) void fe_frames_kernel(const FeArgs a) {
    constexpr int NB = N / 2 + 1, BPL = N / 128;  // bins kept; butterflies per lane and stage
    __shared__ float2 s_tw[N];
    __shared__ float s_re[kFeWaves][N], s_im[kFeWaves][N], s_mag[kFeWaves][NB];
    const int s = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const FeSlot q = fe_slot(a, s);
    const int f0 = blockIdx.x * kFeTile;
    if (f0 >= q.nf) return;  // (the whole workgroup)
    for (int i = threadIdx.x; i < N; i += kFeWaves * 64) s_tw[i] = a.tw[i];
    __syncthreads();
    float *re = s_re[wave], *im = s_im[wave], *mag = s_mag[wave];
    const float *carry = a.carry + (size_t)s * a.L, *audio = a.audio + (size_t)s * a.cs;
    for (int f = f0 + wave; f < min(f0 + kFeTile, q.nf); f += kFeWaves) {
        // frame f covers samples f * step ... f * step + L - 1 of carry ++ chunk
        const int base = f * a.step;
#pragma unroll 4
        for (int n = lane; n < N; n += 64) {
            float v = 0.f;
            if (n < a.L) {
                const int p = base + n;  // < c + k: the frame is complete
                v = (p < q.c ? carry[p] : audio[p - q.c]) * a.window[n];
            }
            re[n] = v, im[n] = 0.f;
        }
        fe_wave_sync();
        // a stage's butterflies touch disjoint pairs: a lane loads its BPL pairs, then stores them; stages are ordered by the sync
#pragma unroll 1
        for (int h = N / 2; h >= 1; h >>= 1) {
            float ar[BPL], ai[BPL], br[BPL], bi[BPL];
            float2 w[BPL];
#pragma unroll
            for (int u = 0; u < BPL; ++u) {
                const int i = lane + 64 * u, j = i & (h - 1), p0 = ((i - j) << 1) + j;
                ar[u] = re[p0], ai[u] = im[p0], br[u] = re[p0 + h], bi[u] = im[p0 + h];
                w[u] = s_tw[h + j];
            }
#pragma unroll
            for (int u = 0; u < BPL; ++u) {
                const int i = lane + 64 * u, j = i & (h - 1), p0 = ((i - j) << 1) + j;
                const float dr = ar[u] - br[u], di = ai[u] - bi[u];
                re[p0] = ar[u] + br[u], im[p0] = ai[u] + bi[u];
                re[p0 + h] = __fmaf_rn(dr, w[u].x, -(di * w[u].y)), im[p0 + h] = __fmaf_rn(dr, w[u].y, di * w[u].x);
            }
            fe_wave_sync();
        }
#pragma unroll 2
        for (int k = lane; k < NB; k += 64) {  // bin k sits at the bit-reversed index
            const int r = (int)(__brev((unsigned)k) >> (32 - a.logN));
            const float xr = re[r], xi = im[r];
            mag[k] = sqrtf(__fmaf_rn(xr, xr, xi * xi));
        }
        fe_wave_sync();
        float *xo = a.x + ((size_t)s * a.NF + f) * a.M;
        for (int j = lane; j < a.M; j += 64) {
            const float *w = a.wt + (size_t)j * a.nbp;
            const int lo = a.blo[j], hi = a.bhi[j];
            float acc = 0.f;
            for (int k = lo; k < hi; ++k) acc = __fmaf_rn(mag[k], w[k], acc);
            xo[j] = (float)log((double)acc + 1e-6);
        }
        fe_wave_sync();  // (the next frame overwrites re / im / mag)
    }
}

__global__ __launch_bounds__(kFeEmitThreads) void fe_emit_kernel(const FeArgs a) {
    __shared__ float s_tmp[kFeMaxLen];
    const int s = blockIdx.x, tid = threadIdx.x;
    const FeSlot q = fe_slot(a, s);
    const int M = a.M, stack = a.stack, G = a.G, F = M * stack;
    float *rows = a.rows + (size_t)s * a.max_rows * F;
    const int h0 = q.rst ? 0 : min(max(a.st_h[s], 0), G - 1);
    const int n0 = q.rst ? 0 : a.st_n[s];
    const int total = h0 + q.nf;  // frames at hand: held ++ new
    int count = 0;
    if (q.live) count = q.fin ? total / stack : (total / G) * a.rm;
    const int emit = count * stack;                          // frames that leave in rows
    const int keep = (q.live && !q.fin) ? total - emit : 0;  // frames held for the next feed (< G)
    float *held = a.held + (size_t)s * G * M;
    const float *x = a.x + (size_t)s * a.NF * M;
    for (int b = tid; b < M; b += kFeEmitThreads) {  // a bin's column is this thread's alone: no hazard between threads
        if (q.live) {
            // the held frames come first.  When anything is emitted in a non-final feed, all of them are (emit >= G > h0); when
            // nothing is, they stay where they are.
            for (int p = 0; p < min(h0, emit); ++p) rows[(size_t)(p / stack) * F + (p % stack) * M + b] = held[(size_t)p * M + b];
            float m = q.rst ? 0.f : a.msum[(size_t)s * M + b];
            int n = n0;
            for (int f = 0; f < q.nf; ++f) {
                const float xv = x[(size_t)f * M + b];
                float y = xv;
                if (a.norm) {
                    n += 1;
                    m += xv;
                    y = xv - (m / (float)n + 1e-8f);
                }
                const int p = h0 + f;
                if (p < emit)
                    rows[(size_t)(p / stack) * F + (p % stack) * M + b] = y;
                else if (p - emit < keep)
                    held[(size_t)(p - emit) * M + b] = y;
            }
            a.msum[(size_t)s * M + b] = q.fin ? 0.f : m;
        }
        for (int r = count; r < a.max_rows; ++r)
            for (int j = 0; j < stack; ++j) rows[(size_t)r * F + j * M + b] = 0.f;
    }
    // the new carry: the last c' = avail - nf * step samples of carry ++ chunk, staged so that every read of the old carry
    // comes before any write of the new one
    const int avail = q.c + q.k;
    const int c1 = (q.live && !q.fin) ? avail - q.nf * a.step : 0;  // < L
    float *carry = a.carry + (size_t)s * a.L;
    const float *audio = a.audio + (size_t)s * a.cs;
    const int src0 = avail - c1;
    for (int i = tid; i < c1; i += kFeEmitThreads) {
        const int p = src0 + i;
        s_tmp[i] = p < q.c ? carry[p] : audio[p - q.c];
    }
    __syncthreads();  // (also: every thread has read the state words)
    if (q.live) {
        for (int i = tid; i < c1; i += kFeEmitThreads) carry[i] = s_tmp[i];
        if (tid == 0) {
            a.st_c[s] = c1;
            a.st_h[s] = keep;
            a.st_n[s] = q.fin ? 0 : (a.norm ? n0 + q.nf : n0);
            a.st_fin[s] = q.fin ? 1 : 0;
        }
    }
    if (tid == 0) a.counts[s] = count;
}

namespace {

FeArgs fe_args(const FeLayout &l, void *workspace) {
    char *w = (char *)workspace;
    FeArgs a{};
    a.window = (const float *)(w + l.window), a.wt = (const float *)(w + l.wt);
    a.blo = (const int *)(w + l.blo), a.bhi = (const int *)(w + l.bhi), a.tw = (const float2 *)(w + l.tw);
    int *st = (int *)(w + l.state);
    a.st_c = st, a.st_n = st + l.S, a.st_h = st + 2 * l.S, a.st_fin = st + 3 * l.S;
    a.msum = (float *)(w + l.msum), a.carry = (float *)(w + l.carry), a.held = (float *)(w + l.held), a.x = (float *)(w + l.x);
    a.S = l.S, a.L = l.L, a.step = l.step, a.M = l.M, a.stack = l.stack, a.rm = l.rm, a.G = l.G, a.logN = l.logN, a.nbp = l.nbp;
    a.NF = l.NF, a.max_rows = l.max_rows;
    return a;
}

template <int N>
hipError_t fe_launch_frames(const FeArgs &a, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL(fe_frames_kernel<N>, grid, dim3(kFeWaves * 64), 0, s, a);
    return hipGetLastError();
}

}  // namespace

bool frontend_layout_ok(int K, int S, int L, int step, int M, int stack, int rm, size_t *bytes, int *max_rows) {
    FeLayout l;
    if (!make_fe_layout(K, S, L, step, M, stack, rm, &l)) return false;
    if (bytes) *bytes = l.bytes;
    if (max_rows) *max_rows = l.max_rows;
    return true;
}

hipError_t launch_frontend_begin(const float *window, const float *mel_weights, int K, int S, int L, int step, int M, int stack,
                                 int rm, void *workspace, hipStream_t s) {
    FeLayout l;
    if (!make_fe_layout(K, S, L, step, M, stack, rm, &l)) return hipErrorInvalidValue;
    char *w = (char *)workspace;
    FePack p{};
    p.window_in = window, p.mel_in = mel_weights;
    p.window = (float *)(w + l.window), p.wt = (float *)(w + l.wt), p.blo = (int *)(w + l.blo), p.bhi = (int *)(w + l.bhi);
    p.tw = (float2 *)(w + l.tw), p.state = (int *)(w + l.state);
    p.zero = (float *)(w + l.msum), p.zero_n = (l.x - l.msum) / sizeof(float);  // msum, carry, held
    p.S = S, p.L = L, p.M = M, p.N = l.N, p.nb = l.nb, p.nbp = l.nbp;
    hipLaunchKernelGGL(fe_pack_kernel, dim3(256), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_frontend_feed(const float *audio, int cs, const int *samples, const int *reset, const int *final_, int norm,
                                float *rows, int *counts, int K, int S, int L, int step, int M, int stack, int rm, void *workspace,
                                hipStream_t s) {
    FeLayout l;
    if (!make_fe_layout(K, S, L, step, M, stack, rm, &l) || cs < 0 || cs > K) return hipErrorInvalidValue;
    FeArgs a = fe_args(l, workspace);
    a.audio = audio, a.cs = cs, a.samples = samples, a.reset = reset, a.final_ = final_, a.norm = norm, a.rows = rows, a.counts = counts;
    const int nf = cs >= 1 ? 1 + (cs - 1) / step : 0;  // the frames this call can complete in a slot
    if (nf > 0) {
        const dim3 grid((nf + kFeTile - 1) / kFeTile, S);
        hipError_t e;
        switch (l.N) {
            case 256: e = fe_launch_frames<256>(a, grid, s); break;
            case 512: e = fe_launch_frames<512>(a, grid, s); break;
            case 1024: e = fe_launch_frames<1024>(a, grid, s); break;
            default: e = fe_launch_frames<2048>(a, grid, s); break;
        }
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(fe_emit_kernel, dim3(S), dim3(kFeEmitThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace rnnt
