// tdt_stream_kernels.hip -- greedy decoding of a token-and-duration (TDT) transducer over a stream of chunks per slot
// (include/rnnt_tdt_stream.h): the greedy stream of greedy_kernels.hip with the step rule of tdt_greedy_kernels.hip.
//   begin   the W2 operand image over all R = V + D columns (launch_greedy_w2), W1 / b1 into the workspace with every slot finished
//           (launch_greedy_stream_pack), then tdt_stream_begin_kernel: the duration set, which arrives as kernel arguments, the
//           place of the frame bases, and every frame base 0.
//   feed    the chunk through W1 + b1 (launch_greedy_stream_proj: one FMA chain per output, so a frame's enc_proj does not depend
//           on the chunking, the slot or S), then tdt_stream_feed_kernel: the row flags of the chunk's frames as
//           greedy_stream_feed_body.h computes them and, in workgroup 0, every slot's state moved on to the chunk.  What a
//           duration jump reached beyond the chunk a slot held is carried: the slot starts the new chunk at frame
//           skip = max(t - Tb, 0), and a slot whose carry exceeds the new chunk too idles through it and carries the rest on.
//   step    tdt_greedy_step_kernel<DT> (tdt_greedy_kernels.hip, launched through launch_tdt_greedy_step_kernel: reused, not
//           copied), then tdt_stream_update_kernel: the update body of tdt_greedy_common.h with hyp_frames = frame base + t.
// Workspace: the TDT greedy workspace at (max_chunk_frames, slots), then W1 [H][J] and b1 [J] as the greedy stream keeps them, then
// the frame bases [slots].  The step takes no enc_width, so begin leaves the frame bases' place (in words past the TDT greedy
// workspace) in the word after the duration set, which the layout reserves (kTdtStreamBaseWord).
#include "rnnt_decode.h"
#include "tdt_greedy_common.h"

namespace rnnt {

constexpr int kTsMaxSlots = 1024, kTsMaxWidth = 4096;  // the greedy stream's limits

__global__ __launch_bounds__(256) void tdt_stream_begin_kernel(int *durset, const TdtDurations dur, const int base_words,
                                                               int *frame_base, const int S) {
    if (threadIdx.x < kTdtGreedyMaxD) durset[threadIdx.x] = dur.d[threadIdx.x];
    if (threadIdx.x == 0) durset[kTdtStreamBaseWord] = base_words;
    for (int b = threadIdx.x; b < S; b += 256) frame_base[b] = 0;
}

// the per-frame range flags of the chunk's frames (greedy_stream_feed_body.h); workgroup 0 also moves every slot's state on to
// the chunk by the rule of the header, in its order
__global__ __launch_bounds__(256) void tdt_stream_feed_kernel(const GreedyStreamArgs a) {
    const int rows = a.S * a.Te;
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {  // (block-uniform trip count and skip: the barrier below is safe)
        const int s = r / a.Te, t = r - s * a.Te;
        if (t >= gs_frames(a, s)) continue;
        const size_t base = ((size_t)s * a.T + t) * a.J;
        bool big = false;
        for (int j = threadIdx.x; j < a.J; j += 256) big |= exp_tab_out_of_range(a.encraw[base + j]);  // also catches NaN
        big = __syncthreads_or(big);
        if (threadIdx.x == 0) a.rowflag[(size_t)s * a.T + t] = big ? 1 : 0;
    }
    if (blockIdx.x != 0) return;
    bool running = false;
    for (int b = threadIdx.x; b < a.S; b += 256) {
        GreedyState s = a.st[b];
        int skip = 0;
        if (a.reset && a.reset[b] != 0) {
            s.n = 0, s.fin = 0, s.score = 0.0;
            s.maxsym = a.max_symbols ? max(a.max_symbols[b], 0) : INT_MAX;
            s.cap = a.max_per_frame;
            a.frame_base[b] = 0;
        } else {
            a.frame_base[b] += s.Tb;
            skip = max(s.t - s.Tb, 0);  // what the last jump reached beyond the chunk (a finished slot: t = Tb = 0)
        }
        s.nf = 0;
        if (s.fin || s.n >= s.maxsym) {  // finished: nothing more until a reset
            s.fin = 1, s.Tb = 0, s.t = 0, s.done = 1;
        } else {
            s.Tb = gs_frames(a, b);
            s.t = skip;
            if (a.final_ && a.final_[b] != 0) s.fin = 1;  // (after this chunk; a carry beyond it is dropped)
            s.done = s.t >= s.Tb ? 1 : 0;
        }
        a.st[b] = s;
        a.hyp_lengths[b] = s.n;
        a.scores[b] = (float)s.score;
        running |= !s.done;
    }
    running = __syncthreads_or(running);
    if (threadIdx.x == 0) a.all_done[0] = running ? 0 : 1;  // (a full hyps buffer: the next step reports 2)
}

// tail: the end of the TDT greedy workspace
__global__ __launch_bounds__(256) void tdt_stream_update_kernel(const TdtGreedyArgs ta, const int *tail) {
    tdt_greedy_update_body<true>(ta, tail + ta.durset[kTdtStreamBaseWord]);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct TdtStreamLayout {
    TdtGreedyLayout t;
    size_t w1, b1, base, total;
};

static bool make_tdt_stream_layout(int Tc, int S, int H, int J, int Vt, int D, int joint_dtype, TdtStreamLayout &L) {
    if (S < 1 || S > kTsMaxSlots || H < 1 || H > kTsMaxWidth) return false;
    if (!make_tdt_greedy_layout(Tc, S, J, Vt, D, joint_dtype, L.t)) return false;
    L.w1 = L.t.total;
    L.b1 = align_up(L.w1 + (size_t)H * J * sizeof(float), 256);
    L.base = align_up(L.b1 + (size_t)J * sizeof(float), 256);
    L.total = align_up(L.base + (size_t)S * sizeof(int), 256);
    return true;
}

hipError_t tdt_stream_workspace_bytes(int Tc, int S, int H, int J, int Vt, int D, int joint_dtype, size_t *bytes) {
    TdtStreamLayout L;
    if (!make_tdt_stream_layout(Tc, S, H, J, Vt, D, joint_dtype, L)) return hipErrorInvalidValue;
    *bytes = L.total;
    return hipSuccess;
}

hipError_t launch_tdt_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2, int H, int J, int Vt,
                                   const int *durations, int D, int S, int Tc, int joint_dtype, void *workspace, hipStream_t s) {
    TdtStreamLayout L;
    if (!make_tdt_stream_layout(Tc, S, H, J, Vt, D, joint_dtype, L)) return hipErrorInvalidValue;
    TdtGreedyArgs ta = {};
    tdt_greedy_bind(ta, L.t, workspace);
    GreedyArgs &a = ta.g;
    a.B = S, a.T = Tc, a.J = J, a.V = Vt + D;
    const int DT = L.t.g.DT;
    hipError_t e;
    if ((e = launch_greedy_w2(a, DT, W2, b2, s)) != hipSuccess) return e;
    char *ws = (char *)workspace;
    e = launch_greedy_stream_pack(W1, b1, (float *)(ws + L.w1), (float *)(ws + L.b1), H, J, a.st, S, DT == 2 ? b2 : nullptr, a.btab,
                                  Vt + D, s);
    if (e != hipSuccess) return e;
    TdtDurations dur;
    for (int i = 0; i < kTdtGreedyMaxD; ++i) dur.d[i] = i < D ? durations[i] : 0;
    hipLaunchKernelGGL(tdt_stream_begin_kernel, dim3(1), dim3(256), 0, s, ta.durset, dur, (int)((L.base - L.t.total) / sizeof(int)),
                       (int *)(ws + L.base), S);
    return hipGetLastError();
}

hipError_t launch_tdt_stream_feed(const float *enc, int Te, const int *chunk_frames, const int *reset, const int *final_,
                                  const int *max_symbols, int max_per_frame, int *hyp_lengths, float *scores, int *all_done, int H,
                                  int J, int Vt, int D, int S, int Tc, int joint_dtype, void *workspace, hipStream_t s) {
    TdtStreamLayout L;
    if (!make_tdt_stream_layout(Tc, S, H, J, Vt, D, joint_dtype, L) || Te < 0 || Te > Tc) return hipErrorInvalidValue;
    GreedyArgs g = {};
    greedy_bind(g, L.t.g, workspace);
    char *ws = (char *)workspace;
    GreedyStreamArgs a = {};
    a.enc = enc, a.W1 = (const float *)(ws + L.w1), a.b1 = (const float *)(ws + L.b1);
    a.chunk_frames = chunk_frames, a.reset = reset, a.final_ = final_, a.max_symbols = max_symbols;
    a.hyp_lengths = hyp_lengths, a.all_done = all_done, a.scores = scores;
    a.st = g.st, a.rowflag = g.rowflag, a.expE = g.expE, a.encraw = g.encraw;
    a.S = S, a.Te = Te, a.T = Tc, a.H = H, a.J = J, a.max_per_frame = max_per_frame;
    a.frame_base = (int *)(ws + L.base);
    const int rows = S * Te;
    const hipError_t e = launch_greedy_stream_proj(a, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tdt_stream_feed_kernel, dim3(rows > 1 ? (rows < 2048 ? rows : 2048) : 1), dim3(256), 0, s, a);
    return hipGetLastError();
}

// the step needs the TDT greedy workspace alone: it finds the frame bases through the word begin left
hipError_t launch_tdt_stream_step(const float *pred_proj, int *hyps, int *hyp_frames, float *hyp_logp, int max_hyp_len,
                                  int *hyp_lengths, float *scores, int *emitted, int *all_done, float *stats, int J, int Vt, int D,
                                  int S, int Tc, int blank, int joint_dtype, void *workspace, hipStream_t s) {
    TdtGreedyLayout L;
    if (S > kTsMaxSlots || !make_tdt_greedy_layout(Tc, S, J, Vt, D, joint_dtype, L)) return hipErrorInvalidValue;
    TdtGreedyArgs ta = {};
    tdt_greedy_bind(ta, L, workspace);
    ta.Vt = Vt, ta.D = D;
    GreedyArgs &a = ta.g;
    a.pred_proj = pred_proj, a.hyps = hyps, a.hyp_lengths = hyp_lengths, a.scores = scores, a.emitted = emitted;
    a.all_done = all_done, a.stats = stats;
    a.hyp_frames = hyp_frames, a.hyp_logp = hyp_logp;
    a.B = S, a.T = Tc, a.J = J, a.V = Vt + D, a.blank = blank, a.max_hyp_len = max_hyp_len;
    const hipError_t e = launch_tdt_greedy_step_kernel(ta, L.g.DT, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tdt_stream_update_kernel, dim3(1), dim3(256), 0, s, ta, (const int *)((char *)workspace + L.total));
    return hipGetLastError();
}

}  // namespace rnnt
