// greedy_kernels.hip -- batched greedy transducer decoding (utils/decoding.py:21-108 for every utterance of a batch at once).
//
// One decode step evaluates the joint for ONE lattice cell per hypothesis -- frame t_b of utterance b against the prediction
// network's current output -- takes the argmax, and moves the hypothesis on.  Per step, for every hypothesis that is not done:
//   step    (greedy_step_kernel<DT>)  h = tanh(enc_proj[b, t_b] + pred_proj[b]) built straight into the MFMA B-operand image in
//           LDS (32 hypotheses = the 32 columns of v_mfma_f32_32x32x16_f16), logits^T = W2^T . h^T chunk by chunk of 32
//           symbols; epilogue per hypothesis: max logit, argmax (lowest index on ties), sum of exps against the max.  A workgroup
//           owns a fixed slice of the vocabulary (four chunks, one per wave) for every step: W2 is read once per hypothesis
//           tile and step, and the slice a workgroup streams is the same every step.  Out: one partial (max, argmax, sum) per
//           (slice, hypothesis).  Nothing of size [B x V] is written.
//   update  (greedy_update_kernel)  one workgroup: the partials of each hypothesis -> (argmax, max, logsumexp) in float64, the
//           state update (emit / advance the frame / done), the all-done word.  A second launch: the kernel boundary makes the
//           partials visible (no inter-workgroup protocol; DESIGN.md "Batched greedy decoding").  greedy_update_timed_kernel
//           (compute_rnnt_greedy_step_timed) also stores, beside every token, the frame that emitted it and the log-softmax
//           of that decision.
// prepare (greedy_begin_kernel, greedy_w2_f16_kernel or joint_prep_kernel via launch_joint_w2_image), once per decode: e^{2x}
//           tables of enc_proj for all frames, a raw copy of it (the direct-tanh route), the per-frame table-range flag, the W2
//           operand image and bias tables, the per-hypothesis state.
//
// Arithmetic: the (argmax, max logit) pair of a hypothesis is bitwise what compute_rnnt_joint_logits computes for that
// hypothesis alone (minibatch = maxT = maxU = 1): the same h (rnnt_joint_math.h), the same operand roundings and W2 scale, the
// same MFMA chains in the same K order, the same epilogue arithmetic:
//   DT 1  f16 joint (jh_logits_kernel MODE 3): h, W2 rounded to binary16; even k-steps into one accumulator, odd ones into a
//         second, summed; logit = fmaf(acc, log2 e, b2 log2 e) ln 2.
//   DT 0  f32-grade joint, J <= 640 (joint_fwd_kernel): r = (1 - h) / 2 (or h itself when max |W2| > kRFormLimit) and s2 W2 split
//         into binary16 hi + lo; three MFMAs per k-step in one chain; logit = fmaf(acc, m2inv, bh) + bl (b2s tables).
//   DT 2  f32-grade joint, 640 < J <= 704 (joint_phase1s_kernel): h split into hi + lo as the A operand; logit = fmaf(acc, 1/s2, b2).
// The call-wide route switches of those kernels are decided PER HYPOTHESIS here: the direct-tanh route (some |x| beyond
// kExpTabLimit) when this hypothesis's enc_proj row or pred_proj row leaves the table range -- exactly when the single-hypothesis
// logits call would raise its flag.  The h / r form depends on W2 alone and is the same for every hypothesis.
#include "rnnt_decode.h"
#include "greedy_common.h"  // GreedyLayout, make_greedy_layout, greedy_bind

#include <limits.h>
#include <math.h>

namespace rnnt {

// ---------------------------------------------------------------------------------------------
// prepare
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void greedy_begin_kernel(const GreedyArgs a) {
    const int J = a.J, rows = a.B * a.T;
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {  // (block-uniform trip count: the barrier below is safe)
        bool big = false;
        const size_t base = (size_t)r * J;
        for (int j = threadIdx.x; j < J; j += 256) {
            const float x = a.enc_proj[base + j];
            big |= exp_tab_out_of_range(x);  // also catches NaN
            a.expE[base + j] = exp_tab(x);
            a.encraw[base + j] = x;
        }
        big = __syncthreads_or(big);
        if (threadIdx.x == 0) a.rowflag[r] = big ? 1 : 0;
    }
    if (blockIdx.x == 0) {
        for (int b = threadIdx.x; b < a.B; b += 256) {
            GreedyState s;
            s.t = 0, s.n = 0, s.nf = 0;
            s.Tb = min(max(a.frame_lengths[b], 0), a.T);  // out-of-range lengths: clamped into the tensor
            s.maxsym = a.max_symbols ? max(a.max_symbols[b], 0) : INT_MAX;
            s.done = (s.Tb == 0 || s.maxsym == 0) ? 1 : 0;
            s.cap = a.max_per_frame, s.fin = 0;
            s.score = 0.0;
            a.st[b] = s;
        }
        if (a.b2 && a.btab)  // DT 2: the bias as joint_phase1s_kernel reads it
            for (int v = threadIdx.x; v < a.V; v += 256) a.btab[v] = a.b2[v];
    }
}

// DT 1: W2 -> binary16 in the A-fragment order of jh_prep_kernel's W2Tp (lane l of k-step ks holds W2[16 ks + 8 (l >> 5) + 0..7]
// [32 vc + (l & 31)]), zero beyond V; b2 log2 e.  The same conversions as jh_prep_kernel.
__global__ __launch_bounds__(256) void greedy_w2_f16_kernel(const float *W2, const float *b2, const int J, const int V, const int NC,
                                                            gf16 *img, float *b2l) {
    const size_t n = (size_t)NC * 32 * J;
    const int KS = J >> 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int e = (int)(i & 7), v31 = (int)((i >> 3) & 31), hf = (int)((i >> 8) & 1);
        const size_t rest = i >> 9;
        const int ks = (int)(rest % KS), vc = (int)(rest / KS);
        const int j = 16 * ks + 8 * hf + e, v = 32 * vc + v31;
        img[i] = (v < V) ? (gf16)W2[(size_t)j * V + v] : (gf16)0.0f;
    }
    for (int v = blockIdx.x * 256 + threadIdx.x; v < NC * 32; v += gridDim.x * 256) b2l[v] = (v < V) ? b2[v] * kLog2e : 0.f;
}

// ---------------------------------------------------------------------------------------------
// step: grid (NS vocabulary slices, ceil(B / 32) hypothesis tiles), 4 waves.  LDS: the B-operand image of the tile's 32
// hypotheses, [J/16 k-steps][64 lanes][8] binary16 (DT 0 / 2: hi, then lo).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool gr_live(const GreedyState &s, const int max_hyp_len) {
    return !s.done && s.n < min(s.maxsym, max_hyp_len);  // (a full hyps buffer pauses a hypothesis: greedy_update_kernel)
}

template <int DT>
__global__ __launch_bounds__(kGrWaves * 64) void greedy_step_kernel(const GreedyArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_t[32], s_live[32], s_slow[32];
    __shared__ float r_m[kGrWaves * 64], r_s[kGrWaves * 64];
    __shared__ int r_i[kGrWaves * 64];
    __shared__ float stage[DT == 2 ? 32 * 33 : 1];
    const int J = a.J;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slice = blockIdx.x, b0 = blockIdx.y * 32;

    bool live = false;
    if (tid < 32) {
        const int b = b0 + tid;
        int t = 0, slow = 0;
        if (b < a.B) {
            const GreedyState s = a.st[b];
            live = gr_live(s, a.max_hyp_len);
            t = min(max(s.t, 0), a.T - 1);
            if (live) slow = a.rowflag[(size_t)b * a.T + t];
        }
        s_live[tid] = live ? 1 : 0, s_t[tid] = t, s_slow[tid] = slow;
    }
    if (!__syncthreads_or(live)) return;  // a tile of done hypotheses reads and writes nothing
    dec_pred_route(a, J, b0, s_live, s_slow, tid);
    __syncthreads();
    gf16 *hA = (gf16 *)smem, *hL = hA + (size_t)J * 32;
    const bool hform = DT == 0 && a.tflag[1] != 0.f;
    dec_build_h<DT>(a, J, b0, s_live, s_slow, [&](int n) { return (size_t)(b0 + n) * a.T + s_t[n]; }, hform, hA, hL, tid);
    __syncthreads();

    // ---- this wave's chunk of 32 symbols
    const int vc = slice * kGrWaves + wave;
    float bm = -INFINITY, bs = 0.f;
    int bi = INT_MAX;
    if (vc < a.NC) {
        const gf32x16 acc = dec_chunk_acc<DT>(a, vc, hA, hL, stage, lane);
        // epilogue: logits of this lane's hypothesis, in increasing symbol order
        float m2inv, w2inv;
        dec_logit_scales<DT>(a, hform, m2inv, w2inv);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int vv = gr_cdrow(r, half), v = 32 * vc + vv;
            const float l = dec_logit<DT>(a, acc[r], vc, vv, v, m2inv, w2inv);
            if (v < a.V) {  // padding columns take no part
                if (l > bm) {
                    bs = fmaf(bs, __builtin_amdgcn_exp2f((bm - l) * kLog2e), 1.0f);
                    bm = l, bi = v;
                } else {
                    bs += __builtin_amdgcn_exp2f((l - bm) * kLog2e);
                }
            }
        }
    }
    r_m[tid] = bm, r_s[tid] = bs, r_i[tid] = bi;
    __syncthreads();
    if (tid < 32 && s_live[tid]) {  // the 2 kGrWaves partials of hypothesis tid, in a fixed order
        float M = -INFINITY;
        int k = INT_MAX;
        for (int q = 0; q < 2 * kGrWaves; ++q) {
            const int src = (q >> 1) * 64 + tid + 32 * (q & 1);
            if (r_m[src] > M || (r_m[src] == M && r_i[src] < k)) M = r_m[src], k = r_i[src];
        }
        float S = 0.f;
        for (int q = 0; q < 2 * kGrWaves; ++q) {
            const int src = (q >> 1) * 64 + tid + 32 * (q & 1);
            if (r_s[src] > 0.f) S += r_s[src] * __builtin_amdgcn_exp2f((r_m[src] - M) * kLog2e);
        }
        const size_t o = (size_t)slice * a.B + b0 + tid;
        a.part_m[o] = M, a.part_s[o] = S, a.part_i[o] = k;
    }
}

// ---------------------------------------------------------------------------------------------
// update: one workgroup over all hypotheses
// ---------------------------------------------------------------------------------------------
template <bool TIMED>
__device__ __forceinline__ void greedy_update_body(const GreedyArgs a) {
    bool running = false, paused = false;
    for (int b = threadIdx.x; b < a.B; b += 256) {
        GreedyState s = a.st[b];
        int em = -1;
        if (gr_live(s, a.max_hyp_len)) {
            float M = -INFINITY;
            int k = INT_MAX;
            for (int q = 0; q < a.NS; ++q) {
                const float m = a.part_m[(size_t)q * a.B + b];
                const int i = a.part_i[(size_t)q * a.B + b];
                if (m > M || (m == M && i < k)) M = m, k = i;
            }
            double S = 0.0;
            for (int q = 0; q < a.NS; ++q) {
                const float ps = a.part_s[(size_t)q * a.B + b];
                if (ps > 0.f) S += (double)ps * exp((double)a.part_m[(size_t)q * a.B + b] - (double)M);
            }
            const double lse = (double)M + log(S);
            if (a.stats) a.stats[2 * b] = M, a.stats[2 * b + 1] = (float)lse;
            s.score += (double)M - lse;
            if (k == a.blank || k >= a.V) {  // blank (or no finite logit at all): next frame
                s.t += 1, s.nf = 0;
            } else {
                a.hyps[(size_t)b * a.max_hyp_len + s.n] = k;
                if (TIMED) {  // (s.t: the frame of this decision, before the state moves on)
                    a.hyp_frames[(size_t)b * a.max_hyp_len + s.n] = (a.frame_base ? a.frame_base[b] : 0) + s.t;
                    a.hyp_logp[(size_t)b * a.max_hyp_len + s.n] = (float)((double)M - lse);
                }
                s.n += 1, s.nf += 1, em = k;
                if (s.cap > 0 && s.nf >= s.cap) s.t += 1, s.nf = 0;
            }
            if (s.t >= s.Tb || s.n >= s.maxsym) s.done = 1;
            a.st[b] = s;
        }
        a.emitted[b] = em;
        a.hyp_lengths[b] = s.n;
        a.scores[b] = (float)s.score;
        if (!s.done) {
            if (s.n < a.max_hyp_len) running = true;
            else paused = true;
        }
    }
    const int any_running = __syncthreads_or(running), any_paused = __syncthreads_or(paused);
    if (threadIdx.x == 0) a.all_done[0] = any_running ? 0 : (any_paused ? 2 : 1);
}

// (two kernels with names of their own: the code-object audits look a kernel up by its name and expect one)
__global__ __launch_bounds__(256) void greedy_update_kernel(const GreedyArgs a) { greedy_update_body<false>(a); }
__global__ __launch_bounds__(256) void greedy_update_timed_kernel(const GreedyArgs a) { greedy_update_body<true>(a); }

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
bool joint_dtype_supported(int joint_dtype, int J, int V);
hipError_t launch_joint_w2_image(const float *W2, const float *b2, int J, int V, float *tflag, void *W2s, hipStream_t s);

// DT of the step kernel for (joint_dtype, J, V), or -1 when the shape is not taken: joint_dtype 0 on the shapes of the f32-grade
// joint (joint_dtype_supported), joint_dtype 1 on J a multiple of 128 up to 640 and 1 <= V <= 8192 (the vocabulary is padded to
// whole chunks of 32 inside the image; the padding takes no part)
int greedy_dt(int joint_dtype, int J, int V) {
    if (joint_dtype == 0) return joint_dtype_supported(0, J, V) ? (J > 640 ? 2 : 0) : -1;
    if (joint_dtype == 1) return (J >= 128 && J <= 640 && J % 128 == 0 && V >= 1 && V <= 8192) ? 1 : -1;
    return -1;
}

hipError_t greedy_workspace_bytes(int T, int B, int J, int V, int joint_dtype, size_t *bytes) {
    GreedyLayout L;
    if (!make_greedy_layout(T, B, J, V, joint_dtype, L)) return hipErrorInvalidValue;
    *bytes = L.total;
    return hipSuccess;
}

hipError_t launch_greedy_begin(const float *enc_proj, const int *frame_lengths, const int *max_symbols, const float *W2,
                               const float *b2, int J, int V, int B, int T, int max_per_frame, int joint_dtype, void *workspace,
                               hipStream_t s) {
    GreedyLayout L;
    if (!make_greedy_layout(T, B, J, V, joint_dtype, L)) return hipErrorInvalidValue;
    GreedyArgs a = {};
    greedy_bind(a, L, workspace);
    a.enc_proj = enc_proj, a.frame_lengths = frame_lengths, a.max_symbols = max_symbols;
    a.B = B, a.T = T, a.J = J, a.V = V, a.max_per_frame = max_per_frame;
    return launch_greedy_prepare(a, L.DT, W2, b2, s);
}

// the W2 operand image and bias tables, the e^{2x} tables of enc_proj, the per-hypothesis state (a: bound to a workspace, with
// enc_proj, frame_lengths, max_symbols, B, T, J, V, NC and max_per_frame set).  Shared with the beam decoder's begin.
hipError_t launch_greedy_w2(const GreedyArgs &a, int DT, const float *W2, const float *b2, hipStream_t s) {
    if (DT == 1) {
        const size_t n = (size_t)a.NC * 32 * a.J;
        const unsigned grid = (unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
        hipLaunchKernelGGL(greedy_w2_f16_kernel, dim3(grid), dim3(256), 0, s, W2, b2, a.J, a.V, a.NC, a.img, a.btab);
        return hipGetLastError();
    }
    return launch_joint_w2_image(W2, b2, a.J, a.V, (float *)a.tflag, a.img, s);
}

hipError_t launch_greedy_prepare(const GreedyArgs &ga, int DT, const float *W2, const float *b2, hipStream_t s) {
    GreedyArgs a = ga;
    const int B = a.B, T = a.T;
    a.b2 = DT == 2 ? b2 : nullptr;
    hipError_t e;
    if ((e = launch_greedy_w2(a, DT, W2, b2, s)) != hipSuccess) return e;
    const int rows = B * T;
    hipLaunchKernelGGL(greedy_begin_kernel, dim3(rows < 2048 ? rows : 2048), dim3(256), 0, s, a);
    return hipGetLastError();
}

template <int DT>
static hipError_t launch_step_dt(const GreedyArgs &a, size_t shm, hipStream_t s) {
    const hipError_t e = set_lds(greedy_step_kernel<DT>, shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(greedy_step_kernel<DT>, dim3(a.NS, (a.B + 31) / 32), dim3(kGrWaves * 64), shm, s, a);
    return hipGetLastError();
}

// hyp_frames != NULL: the timed step (hyp_logp too; frame_base [B] or NULL)
hipError_t launch_greedy_step(const float *pred_proj, int *hyps, int max_hyp_len, int *hyp_lengths, float *scores, int *emitted,
                              int *all_done, float *stats, int *hyp_frames, float *hyp_logp, const int *frame_base, int J, int V,
                              int B, int T, int blank, int joint_dtype, void *workspace, hipStream_t s) {
    GreedyLayout L;
    if (!make_greedy_layout(T, B, J, V, joint_dtype, L)) return hipErrorInvalidValue;
    GreedyArgs a = {};
    greedy_bind(a, L, workspace);
    a.pred_proj = pred_proj, a.hyps = hyps, a.hyp_lengths = hyp_lengths, a.scores = scores, a.emitted = emitted;
    a.all_done = all_done, a.stats = stats;
    a.hyp_frames = hyp_frames, a.hyp_logp = hyp_logp, a.frame_base = frame_base;
    a.B = B, a.T = T, a.J = J, a.V = V, a.blank = blank, a.max_hyp_len = max_hyp_len;
    hipError_t e;
    const size_t shm = (size_t)J * 32 * sizeof(gf16) * (L.DT == 1 ? 1 : 2);
    if (L.DT == 1) e = launch_step_dt<1>(a, shm, s);
    else if (L.DT == 0) e = launch_step_dt<0>(a, shm, s);
    else e = launch_step_dt<2>(a, shm, s);
    if (e != hipSuccess) return e;
    if (hyp_frames) hipLaunchKernelGGL(greedy_update_timed_kernel, dim3(1), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(greedy_update_kernel, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// stream: greedy search over a stream of chunks per slot (include/rnnt.h compute_rnnt_greedy_stream_*).  The workspace is the
// greedy workspace with T = max_chunk_frames and B = slots, then W1 [H][J] and b1 [J]: greedy_step_kernel and
// greedy_update_kernel run on it unchanged.  A feed refills the tables for the chunk's frames and resets every slot's frame
// cursor; a slot that has used up its chunk is done for the step loop until the next feed.
// ---------------------------------------------------------------------------------------------
constexpr int kGsRows = 32, kGsKc = 64;

// enc_proj = enc W1 + b1 for the chunk's frames: a workgroup owns 64 columns (one per lane) and 32 encoder rows (8 per wave);
// every output is one FMA chain over k = 0 ... H-1 in order, then + b1, so it depends on the frame alone (not on the chunking,
// the slot or S).  Out: the raw copy and the e^{2x} table of the frames t < chunk_frames[s].
__global__ __launch_bounds__(256) void greedy_stream_proj_kernel(const GreedyStreamArgs a) {
    __shared__ float xs[kGsRows][kGsKc];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = blockIdx.x * 64 + lane, m0 = blockIdx.y * kGsRows, M = a.S * a.Te;
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < a.H; k0 += kGsKc) {
        for (int i = tid; i < kGsRows * kGsKc; i += 256) {
            const int rr = i / kGsKc, kk = i % kGsKc, m = m0 + rr, k = k0 + kk;
            xs[rr][kk] = (m < M && k < a.H) ? a.enc[(size_t)m * a.H + k] : 0.f;
        }
        __syncthreads();
        const int kn = min(kGsKc, a.H - k0);
        const float *w = a.W1 + (size_t)k0 * a.J + min(col, a.J - 1);
#pragma unroll 4
        for (int kk = 0; kk < kn; ++kk) {
            const float wv_ = w[(size_t)kk * a.J];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = fmaf(xs[wv + 4 * i][kk], wv_, acc[i]);
        }
        __syncthreads();
    }
    if (col >= a.J) return;
    const float bias = a.b1[col];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int m = m0 + wv + 4 * i;
        if (m >= M) continue;
        const int s = m / a.Te, t = m - s * a.Te;
        if (t >= gs_frames(a, s)) continue;
        const float x = acc[i] + bias;
        const size_t o = ((size_t)s * a.T + t) * a.J + col;
        a.encraw[o] = x;
        a.expE[o] = exp_tab(x);
    }
}

#define GREEDY_STREAM_FEED_KERNEL greedy_stream_feed_kernel
#define GREEDY_STREAM_FEED_TIMED 0
#include "greedy_stream_feed_body.h"
#undef GREEDY_STREAM_FEED_KERNEL
#undef GREEDY_STREAM_FEED_TIMED
#define GREEDY_STREAM_FEED_KERNEL greedy_stream_feed_timed_kernel
#define GREEDY_STREAM_FEED_TIMED 1
#include "greedy_stream_feed_body.h"
#undef GREEDY_STREAM_FEED_KERNEL
#undef GREEDY_STREAM_FEED_TIMED

// begin: W1 / b1 into the workspace, every slot finished
__global__ __launch_bounds__(256) void greedy_stream_begin_kernel(const float *W1, const float *b1, float *w1, float *bb1, int H, int J,
                                                                  GreedyState *st, int S, const float *b2, float *btab, int V) {
    const size_t n = (size_t)H * J;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) w1[i] = W1[i];
    if (blockIdx.x != 0) return;
    for (int j = threadIdx.x; j < J; j += 256) bb1[j] = b1[j];
    for (int b = threadIdx.x; b < S; b += 256) {
        GreedyState s;
        s.t = 0, s.n = 0, s.nf = 0, s.done = 1, s.Tb = 0, s.maxsym = 0, s.cap = 0, s.fin = 1;
        s.score = 0.0;
        st[b] = s;
    }
    if (b2 && btab)  // DT 2: the bias as joint_phase1s_kernel reads it
        for (int v = threadIdx.x; v < V; v += 256) btab[v] = b2[v];
}

// the launches the beam stream shares (beam_kernels.hip): W1 / b1 into a workspace with every slot's state finished, and the
// chunk projection
hipError_t launch_greedy_stream_pack(const float *W1, const float *b1, float *w1, float *bb1, int H, int J, GreedyState *st, int S,
                                     const float *b2, float *btab, int V, hipStream_t s) {
    const size_t n = (size_t)H * J;
    const unsigned grid = (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(greedy_stream_begin_kernel, dim3(grid), dim3(256), 0, s, W1, b1, w1, bb1, H, J, st, S, b2, btab, V);
    return hipGetLastError();
}

hipError_t launch_greedy_stream_proj(const GreedyStreamArgs &a, hipStream_t s) {
    const int rows = a.S * a.Te;
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(greedy_stream_proj_kernel, dim3((a.J + 63) / 64, (rows + kGsRows - 1) / kGsRows), dim3(256), 0, s, a);
    return hipGetLastError();
}

constexpr int kGsMaxSlots = 1024, kGsMaxWidth = 4096;

static bool make_stream_layout(int Tc, int S, int H, int J, int V, int joint_dtype, GreedyLayout &L, size_t &w1, size_t &b1) {
    if (S < 1 || S > kGsMaxSlots || H < 1 || H > kGsMaxWidth) return false;
    if (!make_greedy_layout(Tc, S, J, V, joint_dtype, L)) return false;
    w1 = L.total;
    b1 = align_up(w1 + (size_t)H * J * sizeof(float), 256);
    L.total = align_up(b1 + (size_t)J * sizeof(float), 256);
    return true;
}

hipError_t greedy_stream_workspace_bytes(int Tc, int S, int H, int J, int V, int joint_dtype, size_t *bytes) {
    GreedyLayout L;
    size_t w1, b1;
    if (!make_stream_layout(Tc, S, H, J, V, joint_dtype, L, w1, b1)) return hipErrorInvalidValue;
    *bytes = L.total;
    return hipSuccess;
}

hipError_t launch_greedy_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2, int H, int J, int V, int S,
                                      int Tc, int joint_dtype, void *workspace, hipStream_t s) {
    GreedyLayout L;
    size_t w1, bo;
    if (!make_stream_layout(Tc, S, H, J, V, joint_dtype, L, w1, bo)) return hipErrorInvalidValue;
    GreedyArgs a = {};
    greedy_bind(a, L, workspace);
    a.B = S, a.T = Tc, a.J = J, a.V = V;
    hipError_t e;
    if ((e = launch_greedy_w2(a, L.DT, W2, b2, s)) != hipSuccess) return e;
    char *ws = (char *)workspace;
    return launch_greedy_stream_pack(W1, b1, (float *)(ws + w1), (float *)(ws + bo), H, J, a.st, S, L.DT == 2 ? b2 : nullptr, a.btab,
                                     V, s);
}

hipError_t launch_greedy_stream_feed(const float *enc, int Te, const int *chunk_frames, const int *reset, const int *final_,
                                     const int *max_symbols, int max_per_frame, int *hyp_lengths, float *scores, int *all_done,
                                     int *frame_base, int H, int J, int V, int S, int Tc, int joint_dtype, void *workspace,
                                     hipStream_t s) {
    GreedyLayout L;
    size_t w1, bo;
    if (!make_stream_layout(Tc, S, H, J, V, joint_dtype, L, w1, bo) || Te < 0 || Te > Tc) return hipErrorInvalidValue;
    GreedyArgs g = {};
    greedy_bind(g, L, workspace);
    char *ws = (char *)workspace;
    GreedyStreamArgs a = {};
    a.enc = enc, a.W1 = (const float *)(ws + w1), a.b1 = (const float *)(ws + bo);
    a.chunk_frames = chunk_frames, a.reset = reset, a.final_ = final_, a.max_symbols = max_symbols;
    a.hyp_lengths = hyp_lengths, a.all_done = all_done, a.scores = scores;
    a.st = g.st, a.rowflag = g.rowflag, a.expE = g.expE, a.encraw = g.encraw;
    a.S = S, a.Te = Te, a.T = Tc, a.H = H, a.J = J, a.max_per_frame = max_per_frame;
    a.frame_base = frame_base;  // (NULL: the untimed feed)
    const int rows = S * Te;
    const hipError_t e = launch_greedy_stream_proj(a, s);
    if (e != hipSuccess) return e;
    const dim3 grid(rows > 1 ? (rows < 2048 ? rows : 2048) : 1);
    if (frame_base) hipLaunchKernelGGL(greedy_stream_feed_timed_kernel, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(greedy_stream_feed_kernel, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace rnnt
