// tdt_greedy_kernels.hip -- batched greedy decoding of a token-and-duration (TDT) transducer (include/rnnt_tdt_greedy.h): the step
// of greedy_kernels.hip with two heads.  The joint has R = V + D columns: V token logits, then D duration logits.  One decode step
// evaluates the joint for ONE lattice cell per hypothesis, takes the argmax of each head, and moves the hypothesis on by the
// chosen duration.  Per step, for every hypothesis that is not done:
//   step    (tdt_greedy_step_kernel<DT>)  the grid, the tiling and the MFMA chains of greedy_step_kernel over the NC = ceil(R / 32)
//           chunks (rnnt_decode.h, unchanged: every logit is bitwise that of compute_rnnt_joint_logits with alphabet_size = R for
//           the hypothesis alone).  The epilogue keeps TWO running (max, argmax, sum of exps) triples per lane: columns v < V feed
//           the token triple, columns V <= v < R the duration triple (its argmax counts from V).  The duration columns lie in at
//           most two chunks, which may belong to two waves or -- when the span crosses a slice boundary -- to two workgroups, so
//           BOTH heads' partials are written per (slice, hypothesis); a slice without a column of a head writes the empty partial
//           (-inf, INT_MAX, 0).  Nothing of size [B x R] is written.
//   update  (tdt_greedy_update_kernel)  one workgroup: both heads' partials of each hypothesis in slice order -> (argmax, max,
//           logsumexp in float64) per head, the state machine of the header, the all-done word.  The kernel boundary is the only
//           synchronisation between step and update.
// prepare  the greedy decoder's (launch_greedy_prepare with V = R: the W2 operand image over all R columns, the e^{2x} tables, the
//           raw copy, the row flags, the state reset), then tdt_greedy_begin_kernel: the duration set, which arrives as kernel
//           arguments, into the workspace for the update kernel of every later step.
// Workspace: the greedy workspace at alphabet_size = R, then the duration head's partials [NS][B] (max, sum, argmax) and the
// duration set.  The token head's partials live where the greedy decoder keeps its own.
#include "rnnt_decode.h"
#include "tdt_greedy_common.h"  // TdtGreedyArgs, TdtGreedyLayout, the update kernel's body

namespace rnnt {

__global__ __launch_bounds__(64) void tdt_greedy_begin_kernel(int *durset, const TdtDurations dur) {
    if (threadIdx.x < kTdtGreedyMaxD) durset[threadIdx.x] = dur.d[threadIdx.x];
}

// one column into a running (max, argmax, sum) triple: the arithmetic of greedy_step_kernel's epilogue
__device__ __forceinline__ void tg_feed(const float l, const int v, float &bm, float &bs, int &bi) {
    if (l > bm) {
        bs = fmaf(bs, __builtin_amdgcn_exp2f((bm - l) * kLog2e), 1.0f);
        bm = l, bi = v;
    } else {
        bs += __builtin_amdgcn_exp2f((l - bm) * kLog2e);
    }
}

// the 2 kGrWaves partials of hypothesis n of the tile, in a fixed order -> one partial
__device__ __forceinline__ void tg_combine(const float *r_m, const float *r_s, const int *r_i, const int n, float &M, float &S, int &k) {
    M = -INFINITY, k = INT_MAX;
    for (int q = 0; q < 2 * kGrWaves; ++q) {
        const int src = (q >> 1) * 64 + n + 32 * (q & 1);
        if (r_m[src] > M || (r_m[src] == M && r_i[src] < k)) M = r_m[src], k = r_i[src];
    }
    S = 0.f;
    for (int q = 0; q < 2 * kGrWaves; ++q) {
        const int src = (q >> 1) * 64 + n + 32 * (q & 1);
        if (r_s[src] > 0.f) S += r_s[src] * __builtin_amdgcn_exp2f((r_m[src] - M) * kLog2e);
    }
}

// ---------------------------------------------------------------------------------------------
// step: grid (NS slices of the R columns, ceil(B / 32) hypothesis tiles), 4 waves.  LDS: the B-operand image of the tile's 32
// hypotheses, as greedy_step_kernel's.
// ---------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(kGrWaves * 64) void tdt_greedy_step_kernel(const TdtGreedyArgs ta) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_t[32], s_live[32], s_slow[32];
    __shared__ float r_m[kGrWaves * 64], r_s[kGrWaves * 64], q_m[kGrWaves * 64], q_s[kGrWaves * 64];
    __shared__ int r_i[kGrWaves * 64], q_i[kGrWaves * 64];
    __shared__ float stage[DT == 2 ? 32 * 33 : 1];
    const GreedyArgs &a = ta.g;
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
            live = tg_live(s, a.max_hyp_len);
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

    // ---- this wave's chunk of 32 columns: tokens below Vt, durations from Vt to R, padding beyond
    const int vc = slice * kGrWaves + wave;
    float bm = -INFINITY, bs = 0.f, dm = -INFINITY, ds = 0.f;
    int bi = INT_MAX, di = INT_MAX;
    if (vc < a.NC) {
        const gf32x16 acc = dec_chunk_acc<DT>(a, vc, hA, hL, stage, lane);
        float m2inv, w2inv;
        dec_logit_scales<DT>(a, hform, m2inv, w2inv);
#pragma unroll
        for (int r = 0; r < 16; ++r) {  // in increasing column order
            const int vv = gr_cdrow(r, half), v = 32 * vc + vv;
            const float l = dec_logit<DT>(a, acc[r], vc, vv, v, m2inv, w2inv);
            if (v < ta.Vt) tg_feed(l, v, bm, bs, bi);
            else if (v < a.V) tg_feed(l, v - ta.Vt, dm, ds, di);
        }
    }
    r_m[tid] = bm, r_s[tid] = bs, r_i[tid] = bi;
    q_m[tid] = dm, q_s[tid] = ds, q_i[tid] = di;
    __syncthreads();
    if (tid < 32 && s_live[tid]) {
        const size_t o = (size_t)slice * a.B + b0 + tid;
        float M, S;
        int k;
        tg_combine(r_m, r_s, r_i, tid, M, S, k);
        a.part_m[o] = M, a.part_s[o] = S, a.part_i[o] = k;
        tg_combine(q_m, q_s, q_i, tid, M, S, k);
        ta.dpart_m[o] = M, ta.dpart_s[o] = S, ta.dpart_i[o] = k;
    }
}

// ---------------------------------------------------------------------------------------------
// update: one workgroup over all hypotheses
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tdt_greedy_update_kernel(const TdtGreedyArgs ta) {
    tdt_greedy_update_body<false>(ta, nullptr);  // (tdt_greedy_common.h)
}

// ---------------------------------------------------------------------------------------------
// host side (the layout and its binding: tdt_greedy_common.h)
// ---------------------------------------------------------------------------------------------
hipError_t tdt_greedy_workspace_bytes(int T, int B, int J, int Vt, int D, int joint_dtype, size_t *bytes) {
    TdtGreedyLayout L;
    if (!make_tdt_greedy_layout(T, B, J, Vt, D, joint_dtype, L)) return hipErrorInvalidValue;
    *bytes = L.total;
    return hipSuccess;
}

hipError_t launch_tdt_greedy_begin(const float *enc_proj, const int *frame_lengths, const int *max_symbols, const float *W2,
                                   const float *b2, int J, int Vt, const int *durations, int D, int B, int T, int max_per_frame,
                                   int joint_dtype, void *workspace, hipStream_t s) {
    TdtGreedyLayout L;
    if (!make_tdt_greedy_layout(T, B, J, Vt, D, joint_dtype, L)) return hipErrorInvalidValue;
    TdtGreedyArgs ta = {};
    tdt_greedy_bind(ta, L, workspace);
    GreedyArgs &a = ta.g;
    a.enc_proj = enc_proj, a.frame_lengths = frame_lengths, a.max_symbols = max_symbols;
    a.B = B, a.T = T, a.J = J, a.V = Vt + D, a.max_per_frame = max_per_frame;
    const hipError_t e = launch_greedy_prepare(a, L.g.DT, W2, b2, s);
    if (e != hipSuccess) return e;
    TdtDurations dur;
    for (int i = 0; i < kTdtGreedyMaxD; ++i) dur.d[i] = i < D ? durations[i] : 0;
    hipLaunchKernelGGL(tdt_greedy_begin_kernel, dim3(1), dim3(64), 0, s, ta.durset, dur);
    return hipGetLastError();
}

template <int DT>
static hipError_t launch_tdt_step_dt(const TdtGreedyArgs &ta, size_t shm, hipStream_t s) {
    const hipError_t e = set_lds(tdt_greedy_step_kernel<DT>, shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tdt_greedy_step_kernel<DT>, dim3(ta.g.NS, (ta.g.B + 31) / 32), dim3(kGrWaves * 64), shm, s, ta);
    return hipGetLastError();
}

// the step kernel alone (the stream's translation unit runs an update kernel of its own after it)
hipError_t launch_tdt_greedy_step_kernel(const TdtGreedyArgs &ta, int DT, hipStream_t s) {
    const size_t shm = (size_t)ta.g.J * 32 * sizeof(gf16) * (DT == 1 ? 1 : 2);
    if (DT == 1) return launch_tdt_step_dt<1>(ta, shm, s);
    if (DT == 0) return launch_tdt_step_dt<0>(ta, shm, s);
    return launch_tdt_step_dt<2>(ta, shm, s);
}

// hyp_frames / hyp_logp: both given or both NULL
hipError_t launch_tdt_greedy_step(const float *pred_proj, int *hyps, int *hyp_frames, float *hyp_logp, int max_hyp_len,
                                  int *hyp_lengths, float *scores, int *emitted, int *all_done, float *stats, int J, int Vt, int D,
                                  int B, int T, int blank, int joint_dtype, void *workspace, hipStream_t s) {
    TdtGreedyLayout L;
    if (!make_tdt_greedy_layout(T, B, J, Vt, D, joint_dtype, L)) return hipErrorInvalidValue;
    TdtGreedyArgs ta = {};
    tdt_greedy_bind(ta, L, workspace);
    ta.Vt = Vt, ta.D = D;
    GreedyArgs &a = ta.g;
    a.pred_proj = pred_proj, a.hyps = hyps, a.hyp_lengths = hyp_lengths, a.scores = scores, a.emitted = emitted;
    a.all_done = all_done, a.stats = stats;
    a.hyp_frames = hyp_frames, a.hyp_logp = hyp_logp;
    a.B = B, a.T = T, a.J = J, a.V = Vt + D, a.blank = blank, a.max_hyp_len = max_hyp_len;
    const hipError_t e = launch_tdt_greedy_step_kernel(ta, L.g.DT, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tdt_greedy_update_kernel, dim3(1), dim3(256), 0, s, ta);
    return hipGetLastError();
}

}  // namespace rnnt
