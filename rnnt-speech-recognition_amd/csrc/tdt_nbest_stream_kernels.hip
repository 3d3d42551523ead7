// tdt_nbest_stream_kernels.hip -- beam search of a token-and-duration (TDT) transducer over a stream of chunks per slot
// (include/rnnt_tdt_beam_stream.h): the beam stream of beam_kernels.hip with the rule of tdt_beam_kernels.hip.
//   begin    the W2 operand image over all R = V + D columns (launch_greedy_w2), W1 / b1 into the workspace with every slot finished
//            (launch_greedy_stream_pack), then tdt_beam_stream_begin_kernel: every beam empty, the duration set, which arrives as
//            kernel arguments, the place of the frame bases and every frame base 0.
//   feed     the chunk through W1 + b1 (launch_greedy_stream_proj: one FMA chain per output, so a frame's enc_proj does not depend
//            on the chunking, the slot or S), then tdt_beam_stream_feed_kernel: beam_stream_feed_kernel's shape (the row flags of
//            the chunk's frames; workgroup 0 moves every slot on) plus, per slot, the frame base and the cursors of its occupied
//            hypotheses rebased onto the new chunk.  A hypothesis's cursor (BeamSlot::pad) counts from the first frame of the chunk
//            its slot holds; what a duration jump reached beyond that chunk stays in it across the feed, per hypothesis.
//   step     tdt_beam_stream_step_kernel<DT>: tdt_beam_step_body.h, the offline kernel's text, plus one store per active row (the
//            blank's logit into BeamArgs::bl); then tdt_beam_stream_select_kernel / _timed_kernel: tdt_beam_select_body.h with the
//            full-row rule and {frame base + t, d} in the timed rows.
//   results  the beams best first, cursors and frames from the slot's reset, and both stable prefix lengths.
// Workspace: the TDT beam workspace (tdt_beam_common.h) at (max_chunk_frames, slots, beam) with rows of stride N = max_hyp_len, then
// W1 [H][J] and b1 [J] as the beam stream keeps them, then the frame bases [slots].  Step and results take no enc_width, so begin
// leaves the frame bases' place (in words past the TDT beam workspace) in the word after the duration set (kTdtBeamBaseWord).
#include "rnnt_decode.h"

namespace rnnt {
constexpr int kBeamMax = 16;
constexpr unsigned long long kHashMul = 0x9E3779B97F4A7C15ull;  // beam_kernels.hip's: h' = h kHashMul + (v + 1)
}  // namespace rnnt

#include "tdt_beam_common.h"

namespace rnnt {

constexpr int kTbsMaxRows = 1024, kTbsMaxWidth = 4096;  // the beam stream's limits: S K rows, enc_width

// ---------------------------------------------------------------------------------------------
// begin: every beam empty (the slots' states were set finished by launch_greedy_stream_pack), the duration set, the frame bases
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tdt_beam_stream_begin_kernel(const TdtBeamArgs ta, const TdtBeamDurations dur, const int base_words,
                                                                    int *frame_base) {
    const BeamArgs &a = ta.b;
    if (blockIdx.x == 0 && threadIdx.x < kTdtBeamMaxD) ta.durset[threadIdx.x] = dur.d[threadIdx.x];
    if (blockIdx.x == 0 && threadIdx.x == 0) ta.durset[kTdtBeamBaseWord] = base_words;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < a.R; r += gridDim.x * 256) {
        BeamSlot s;
        s.score = -INFINITY, s.hash = 0, s.len = 0, s.pad = 0;
        a.slot[r] = s;
        if (r % a.K == 0) a.nslot[r / a.K] = 0, frame_base[r / a.K] = 0;
    }
}

// ---------------------------------------------------------------------------------------------
// feed: the per-frame range flags of the chunk's frames (as beam_stream_feed_kernel forms them); workgroup 0 also moves every slot
// on by the rule of the header, in its order
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tdt_beam_stream_feed_kernel(const GreedyStreamArgs a, BeamSlot *slot, int *nslot, const int K) {
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
    for (int b = threadIdx.x; b < a.S; b += 256) {
        GreedyState s = a.st[b];
        if (a.reset && a.reset[b] != 0) {  // a new stream: the beam [((), 0, 0)], no steps taken, no frames behind it
            s.n = 0, s.fin = 0;
            for (int k = 0; k < K; ++k) {
                BeamSlot e;
                e.score = k == 0 ? 0.0 : -INFINITY, e.hash = 0, e.len = 0, e.pad = 0;
                slot[b * K + k] = e;
            }
            nslot[b] = 1;
            a.frame_base[b] = 0;
        } else if (!s.fin) {  // the chunk the slot held is behind it: every occupied hypothesis keeps what it reached beyond it
            const int Tb_old = max(s.Tb, 0), nb = min(max(nslot[b], 0), K);
            a.frame_base[b] += Tb_old;
            for (int k = 0; k < nb; ++k) slot[b * K + k].pad = max(slot[b * K + k].pad - Tb_old, 0);
        }
        s.t = 0, s.nf = 0, s.maxsym = INT_MAX, s.cap = 0, s.score = 0.0;
        if (s.fin) {  // finished: frozen until a reset
            s.Tb = 0;
        } else {
            s.Tb = gs_frames(a, b);
            if (a.final_ && a.final_[b] != 0) s.fin = 1;  // (after this chunk; a carry beyond it is dropped)
        }
        s.done = s.Tb == 0 ? 1 : 0;
        a.st[b] = s;
    }
}

// ---------------------------------------------------------------------------------------------
// step and select: the offline kernels' text (tdt_beam_step_body.h, tdt_beam_select_body.h)
// ---------------------------------------------------------------------------------------------
#define TDT_BEAM_STEP_KERNEL tdt_beam_stream_step_kernel
#define TDT_BEAM_STEP_STREAM 1
#include "tdt_beam_step_body.h"
#undef TDT_BEAM_STEP_KERNEL
#undef TDT_BEAM_STEP_STREAM

#include "tdt_beam_select_body.h"

__global__ __launch_bounds__(256) void tdt_beam_stream_select_kernel(const TdtBeamArgs ta) { tdt_beam_select_body<false, true>(ta); }
__global__ __launch_bounds__(256) void tdt_beam_stream_select_timed_kernel(const TdtBeamArgs ta) { tdt_beam_select_body<true, true>(ta); }

// ---------------------------------------------------------------------------------------------
// results: one workgroup per slot; the current beams, best first, and the stable prefix lengths (beam_results_body's stream path:
// rows 1 ... nb-1 against row 0, position by position; an integer minimum in LDS)
// ---------------------------------------------------------------------------------------------
// PAIR: positions agree only when the emission frame and the duration agree too (the timed stable length)
template <bool PAIR>
__device__ __forceinline__ int tbs_common_prefix(const int *tok, const int2 *tt, const int T, const int nb, const int shortest,
                                                 int *s_first) {
    if (threadIdx.x == 0) *s_first = shortest;
    __syncthreads();
    int first = shortest;
    for (int p = threadIdx.x; p < shortest && first == shortest; p += 256)
        for (int k = 1; k < nb; ++k) {
            bool diff = tok[(size_t)k * T + p] != tok[p];
            if (PAIR) diff |= tt[(size_t)k * T + p].x != tt[p].x || tt[(size_t)k * T + p].y != tt[p].y;
            if (diff) first = p;
        }
    if (first < shortest) atomicMin(s_first, first);  // (LDS)
    __syncthreads();
    return *s_first;
}

template <bool TIMED>
__device__ __forceinline__ void tdt_beam_stream_results_body(const TdtBeamArgs &ta) {
    __shared__ int s_first;
    const BeamArgs &a = ta.b;
    const GreedyArgs &g = a.g;
    const int b = blockIdx.x, K = a.K, T = a.N;
    const int cur = g.st[b].n & 1, nb = min(max(a.nslot[b], 0), K);
    const int fbase = (ta.tail + ta.durset[kTdtBeamBaseWord])[b];
    const int *tok = a.tok + ((size_t)cur * g.B + b) * K * T;
    int shortest = nb > 0 ? INT_MAX : 0;
    for (int k = 0; k < K; ++k) {
        const int n = k < nb ? min(max(a.slot[b * K + k].len, 0), T) : 0;
        if (k < nb) shortest = min(shortest, n);
        for (int p = threadIdx.x; p < T; p += 256) a.hyps[((size_t)b * K + k) * T + p] = p < n ? tok[(size_t)k * T + p] : 0;
        if (TIMED && a.hyp_frames) {
            const int2 *tt = a.tt + (((size_t)cur * g.B + b) * K + k) * T;
            for (int p = threadIdx.x; p < T; p += 256) {
                int ef = -1, ed = -1;
                if (p < n) ef = tt[p].x, ed = tt[p].y;
                a.hyp_frames[((size_t)b * K + k) * T + p] = ef;
                ta.hyp_durations[((size_t)b * K + k) * T + p] = ed;
            }
        }
        if (threadIdx.x == 0) {
            a.hyp_lengths[b * K + k] = n;
            a.scores[b * K + k] = k < nb ? (float)a.slot[b * K + k].score : -INFINITY;
            if (ta.cursors) ta.cursors[b * K + k] = k < nb ? fbase + a.slot[b * K + k].pad : -1;
        }
    }
    if (a.stable) {  // (uniform)
        const int n = tbs_common_prefix<false>(tok, nullptr, T, nb, shortest, &s_first);
        if (threadIdx.x == 0) a.stable[b] = n;
    }
    if (TIMED && a.tstable) {  // (uniform)
        __syncthreads();
        const int n = tbs_common_prefix<true>(tok, a.tt + ((size_t)cur * g.B + b) * K * T, T, nb, shortest, &s_first);
        if (threadIdx.x == 0) a.tstable[b] = n;
    }
}

__global__ __launch_bounds__(256) void tdt_beam_stream_results_kernel(const TdtBeamArgs ta) { tdt_beam_stream_results_body<false>(ta); }
__global__ __launch_bounds__(256) void tdt_beam_stream_results_timed_kernel(const TdtBeamArgs ta) {
    tdt_beam_stream_results_body<true>(ta);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct TdtBeamStreamLayout {
    TdtBeamLayout t;
    size_t w1, b1, base, total;
};

static bool make_tdt_beam_stream_layout(int Tc, int S, int K, int N, int H, int J, int Vt, int D, int joint_dtype, bool timed,
                                        TdtBeamStreamLayout &L) {
    if (S < 1 || K < 1 || K > kBeamMax || (long long)S * K > kTbsMaxRows || H < 1 || H > kTbsMaxWidth) return false;
    if (!make_tdt_beam_layout_n(Tc, S, K, N, J, Vt, D, joint_dtype, timed, L.t)) return false;
    L.w1 = L.t.total;
    L.b1 = align_up(L.w1 + (size_t)H * J * sizeof(float), 256);
    L.base = align_up(L.b1 + (size_t)J * sizeof(float), 256);
    L.total = align_up(L.base + (size_t)S * sizeof(int), 256);
    return (L.base - L.t.total) / sizeof(int) < (1ull << 31);
}

hipError_t tdt_beam_stream_workspace_bytes(int Tc, int S, int K, int N, int H, int J, int Vt, int D, int joint_dtype, bool timed,
                                           size_t *bytes) {
    TdtBeamStreamLayout L;
    if (!make_tdt_beam_stream_layout(Tc, S, K, N, H, J, Vt, D, joint_dtype, timed, L)) return hipErrorInvalidValue;
    *bytes = L.total;
    return hipSuccess;
}

hipError_t launch_tdt_beam_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2, int H, int J, int Vt,
                                        const int *durations, int D, int S, int Tc, int K, int N, int joint_dtype, bool timed,
                                        void *workspace, hipStream_t s) {
    TdtBeamStreamLayout L;
    if (!make_tdt_beam_stream_layout(Tc, S, K, N, H, J, Vt, D, joint_dtype, timed, L)) return hipErrorInvalidValue;
    TdtBeamArgs ta = {};
    if (!tdt_beam_bind_n(ta, Tc, S, K, N, J, Vt, D, joint_dtype, timed, workspace, L.t)) return hipErrorInvalidValue;
    GreedyArgs &g = ta.b.g;
    const int DT = L.t.b.DT;
    hipError_t e;
    if ((e = launch_greedy_w2(g, DT, W2, b2, s)) != hipSuccess) return e;
    char *ws = (char *)workspace;
    e = launch_greedy_stream_pack(W1, b1, (float *)(ws + L.w1), (float *)(ws + L.b1), H, J, g.st, S, DT == 2 ? b2 : nullptr, g.btab,
                                  Vt + D, s);
    if (e != hipSuccess) return e;
    TdtBeamDurations dur;
    for (int i = 0; i < kTdtBeamMaxD; ++i) dur.d[i] = i < D ? durations[i] : 0;
    hipLaunchKernelGGL(tdt_beam_stream_begin_kernel, dim3((ta.b.R + 255) / 256), dim3(256), 0, s, ta, dur,
                       (int)((L.base - L.t.total) / sizeof(int)), (int *)(ws + L.base));
    return hipGetLastError();
}

hipError_t launch_tdt_beam_stream_feed(const float *enc, int Te, const int *chunk_frames, const int *reset, const int *final_, int H,
                                       int J, int Vt, int D, int S, int Tc, int K, int N, int joint_dtype, bool timed, void *workspace,
                                       hipStream_t s) {
    TdtBeamStreamLayout L;
    if (!make_tdt_beam_stream_layout(Tc, S, K, N, H, J, Vt, D, joint_dtype, timed, L) || Te < 0 || Te > Tc) return hipErrorInvalidValue;
    TdtBeamArgs ta = {};
    if (!tdt_beam_bind_n(ta, Tc, S, K, N, J, Vt, D, joint_dtype, timed, workspace, L.t)) return hipErrorInvalidValue;
    const BeamArgs &b = ta.b;
    char *ws = (char *)workspace;
    GreedyStreamArgs a = {};
    a.enc = enc, a.W1 = (const float *)(ws + L.w1), a.b1 = (const float *)(ws + L.b1);
    a.chunk_frames = chunk_frames, a.reset = reset, a.final_ = final_;
    a.st = b.g.st, a.rowflag = b.g.rowflag, a.expE = b.g.expE, a.encraw = b.g.encraw;
    a.S = S, a.Te = Te, a.T = Tc, a.H = H, a.J = J;
    a.frame_base = (int *)(ws + L.base);
    const hipError_t e = launch_greedy_stream_proj(a, s);
    if (e != hipSuccess) return e;
    const int rows = S * Te;
    hipLaunchKernelGGL(tdt_beam_stream_feed_kernel, dim3(rows > 1 ? (rows < 2048 ? rows : 2048) : 1), dim3(256), 0, s, a, b.slot,
                       b.nslot, K);
    return hipGetLastError();
}

template <int DT>
static hipError_t launch_tdt_beam_stream_step_dt(const TdtBeamArgs &ta, size_t shm, hipStream_t s) {
    const hipError_t e = set_lds(tdt_beam_stream_step_kernel<DT>, shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tdt_beam_stream_step_kernel<DT>, dim3(ta.b.g.NS, (ta.b.R + 31) / 32), dim3(kGrWaves * 64), shm, s, ta);
    return hipGetLastError();
}

// step and results need the TDT beam workspace alone: they find the frame bases through the word begin left
hipError_t launch_tdt_beam_stream_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits, int *topk_symbols,
                                       float *dur_logits, float *lse, int J, int Vt, int D, int S, int Tc, int K, int N, int blank,
                                       int joint_dtype, bool timed, void *workspace, hipStream_t s) {
    TdtBeamArgs ta = {};
    TdtBeamLayout L;
    if ((long long)S * K > kTbsMaxRows || !tdt_beam_bind_n(ta, Tc, S, K, N, J, Vt, D, joint_dtype, timed, workspace, L))
        return hipErrorInvalidValue;
    BeamArgs &a = ta.b;
    a.g.pred_proj = pred_proj, a.g.blank = blank;
    a.parents = parents, a.emitted = emitted, a.topl = topk_logits, a.tops = topk_symbols, a.lse = lse;
    ta.durl = dur_logits;
    ta.tail = (const int *)((char *)workspace + L.total);
    hipError_t e;
    const size_t shm = (size_t)J * 32 * sizeof(gf16) * (L.b.DT == 1 ? 1 : 2);
    if (L.b.DT == 1) e = launch_tdt_beam_stream_step_dt<1>(ta, shm, s);
    else if (L.b.DT == 0) e = launch_tdt_beam_stream_step_dt<0>(ta, shm, s);
    else e = launch_tdt_beam_stream_step_dt<2>(ta, shm, s);
    if (e != hipSuccess) return e;
    if (timed) hipLaunchKernelGGL(tdt_beam_stream_select_timed_kernel, dim3(S), dim3(256), 0, s, ta);
    else hipLaunchKernelGGL(tdt_beam_stream_select_kernel, dim3(S), dim3(256), 0, s, ta);
    return hipGetLastError();
}

hipError_t launch_tdt_beam_stream_results(int *hyps, int *hyp_lengths, float *scores, int *cursors, int *stable_lengths,
                                          int *hyp_frames, int *hyp_durations, int *timed_stable_lengths, int J, int Vt, int D, int S,
                                          int Tc, int K, int N, int joint_dtype, bool timed, void *workspace, hipStream_t s) {
    TdtBeamArgs ta = {};
    TdtBeamLayout L;
    if ((long long)S * K > kTbsMaxRows || !tdt_beam_bind_n(ta, Tc, S, K, N, J, Vt, D, joint_dtype, timed, workspace, L))
        return hipErrorInvalidValue;
    BeamArgs &a = ta.b;
    a.hyps = hyps, a.hyp_lengths = hyp_lengths, a.scores = scores, a.stable = stable_lengths;
    a.hyp_frames = hyp_frames, a.tstable = timed_stable_lengths;
    ta.cursors = cursors, ta.hyp_durations = hyp_durations;
    ta.tail = (const int *)((char *)workspace + L.total);
    if (timed) hipLaunchKernelGGL(tdt_beam_stream_results_timed_kernel, dim3(S), dim3(256), 0, s, ta);
    else hipLaunchKernelGGL(tdt_beam_stream_results_kernel, dim3(S), dim3(256), 0, s, ta);
    return hipGetLastError();
}

}  // namespace rnnt
