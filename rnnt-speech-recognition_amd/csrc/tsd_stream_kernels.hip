// tsd_stream_kernels.hip -- the beam search with several symbols per frame (time-synchronous decoding) over a stream of chunks per
// slot (include/rnnt_beam_multi_stream.h): the beam stream of beam_kernels.hip with the rule of include/rnnt_beam_multi.h.
//   begin    the W2 operand image (launch_greedy_w2), W1 / b1 into the workspace with every slot finished
//            (launch_greedy_stream_pack), then tsd_stream_begin_kernel: both lists of every slot empty, every frame base 0.
//   feed     the chunk through W1 + b1 (launch_greedy_stream_proj: one FMA chain per output, so a frame's enc_proj does not depend
//            on the chunking, the slot or S), then tsd_stream_feed_kernel: beam_stream_feed_kernel's shape (the row flags of the
//            chunk's frames; workgroup 0 moves every slot on) plus, per slot, the round (0), the closed list (emptied) and the frame
//            base.
//   step     tsd_stream_step_kernel<DT>: beam_step_body.h at its flag value 3, the text the offline search compiles; then
//            tsd_stream_select_kernel / _timed_kernel: multibeam_select_body.h, the offline select kernel's text, the timed one
//            with a frame row beside every token row.
//   results  list A best first, the stable prefix over A; timed: the frames and the prefix that agrees in token and frame.
// Workspace: the offline search's (multibeam_common.h) at (max_chunk_frames, slots, beam), then the frame bases [slots], then (timed)
// the frame rows [2][slots][2 beam][max_hyp_len], then W1 [H][J] and b1 [J] as the beam stream keeps them.  Step and results take no
// enc_width: nothing they reach lies behind W1.
// No global atomics, no memset; every word of the workspace that is read was written since begin.
#include "rnnt_decode.h"

namespace rnnt {
constexpr int kBeamMax = 16;
constexpr unsigned long long kHashMul = 0x9E3779B97F4A7C15ull;  // beam_kernels.hip's: h' = h kHashMul + (v + 1)
}  // namespace rnnt

#include "multibeam_common.h"

namespace rnnt {

constexpr int kTsdMaxWidth = 4096;  // enc_width, as the beam stream's

// ---------------------------------------------------------------------------------------------
// begin: both lists of every slot empty (the slots' states were set finished by launch_greedy_stream_pack), the frame bases 0
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsd_stream_begin_kernel(const MultiBeamArgs m, int *frame_base) {
    const BeamArgs &a = m.b;
    const int KR = 2 * a.K;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < a.R; r += gridDim.x * 256) {
        BeamSlot s;
        s.score = -INFINITY, s.hash = 0, s.len = 0, s.pad = 0;
        a.slot[r] = s;
        if (r % KR == 0) a.nslot[r / KR] = 0, m.nclosed[r / KR] = 0, frame_base[r / KR] = 0;
    }
}

// ---------------------------------------------------------------------------------------------
// feed: the per-frame range flags of the chunk's frames (as beam_stream_feed_kernel forms them); workgroup 0 also moves every slot
// on by the rule of the header
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsd_stream_feed_kernel(const GreedyStreamArgs a, BeamSlot *slot, int *nslot, int *nclosed,
                                                              const int K) {
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
    const int KR = 2 * K;
    for (int b = threadIdx.x; b < a.S; b += 256) {
        GreedyState s = a.st[b];
        if (a.reset && a.reset[b] != 0) {  // a new stream: A = [((), 0)], B = [], no steps taken, no frames behind it
            s.n = 0, s.fin = 0;
            for (int k = 0; k < KR; ++k) {
                BeamSlot e;
                e.score = k == 0 ? 0.0 : -INFINITY, e.hash = 0, e.len = 0, e.pad = 0;
                slot[b * KR + k] = e;
            }
            nslot[b] = 1;
            a.frame_base[b] = 0;
        } else if (!s.fin) {  // the chunk the slot held is behind it
            a.frame_base[b] += max(s.Tb, 0);
        }
        // round 0 of chunk frame 0 with B = []: what a feed finds unfinished of the last frame's rounds is dropped
        nclosed[b] = 0;
        s.t = 0, s.nf = 0, s.maxsym = INT_MAX, s.cap = 0, s.score = 0.0;
        if (s.fin) {  // finished: frozen until a reset
            s.Tb = 0;
        } else {
            s.Tb = gs_frames(a, b);
            if (a.final_ && a.final_[b] != 0) s.fin = 1;  // (after this chunk)
        }
        s.done = s.Tb == 0 ? 1 : 0;
        a.st[b] = s;
    }
}

// ---------------------------------------------------------------------------------------------
// step and select: the offline kernels' text (beam_step_body.h at flag value 3, multibeam_select_body.h)
// ---------------------------------------------------------------------------------------------
#define BEAM_STEP_KERNEL tsd_stream_step_kernel
#define BEAM_STEP_BIAS 3
#include "beam_step_body.h"
#undef BEAM_STEP_KERNEL
#undef BEAM_STEP_BIAS

#include "multibeam_select_body.h"

__global__ __launch_bounds__(256) void tsd_stream_select_kernel(const MultiBeamArgs m) { multibeam_select_body<false>(m); }
__global__ __launch_bounds__(256) void tsd_stream_select_timed_kernel(const MultiBeamArgs m) { multibeam_select_body<true>(m); }

// ---------------------------------------------------------------------------------------------
// results: one workgroup per slot; list A best first, and the stable prefix lengths (rows 1 ... nA-1 against row 0, position by
// position; an integer minimum in LDS)
// ---------------------------------------------------------------------------------------------
// PAIR: positions agree only when the emission frame agrees too (the timed stable length)
template <bool PAIR>
__device__ __forceinline__ int tsd_common_prefix(const int *tok, const int *frm, const int N, const int nA, const int shortest,
                                                 int *s_first) {
    if (threadIdx.x == 0) *s_first = shortest;
    __syncthreads();
    int first = shortest;
    for (int p = threadIdx.x; p < shortest && first == shortest; p += 256)
        for (int k = 1; k < nA; ++k) {
            bool diff = tok[(size_t)k * N + p] != tok[p];
            if (PAIR) diff |= frm[(size_t)k * N + p] != frm[p];
            if (diff) first = p;
        }
    if (first < shortest) atomicMin(s_first, first);  // (LDS)
    __syncthreads();
    return *s_first;
}

template <bool TIMED>
__device__ __forceinline__ void tsd_stream_results_body(const MultiBeamArgs &m) {
    __shared__ int s_first;
    const BeamArgs &a = m.b;
    const GreedyArgs &g = a.g;
    const int b = blockIdx.x, K = a.K, KR = 2 * K, N = a.N;
    const int cur = g.st[b].n & 1, nA = min(max(a.nslot[b], 0), K);
    const int *tok = a.tok + ((size_t)cur * g.B + b) * KR * N;
    const int *frm = TIMED ? m.frm + ((size_t)cur * g.B + b) * KR * N : nullptr;
    int shortest = nA > 0 ? INT_MAX : 0;
    for (int k = 0; k < K; ++k) {
        const int n = k < nA ? min(max(a.slot[b * KR + k].len, 0), N) : 0;
        if (k < nA) shortest = min(shortest, n);
        for (int p = threadIdx.x; p < N; p += 256) a.hyps[((size_t)b * K + k) * N + p] = p < n ? tok[(size_t)k * N + p] : 0;
        if (TIMED && a.hyp_frames)
            for (int p = threadIdx.x; p < N; p += 256) a.hyp_frames[((size_t)b * K + k) * N + p] = p < n ? frm[(size_t)k * N + p] : -1;
        if (threadIdx.x == 0) {
            a.hyp_lengths[b * K + k] = n;
            a.scores[b * K + k] = k < nA ? (float)a.slot[b * KR + k].score : -INFINITY;
        }
    }
    if (a.stable) {  // (uniform)
        const int n = tsd_common_prefix<false>(tok, nullptr, N, nA, shortest, &s_first);
        if (threadIdx.x == 0) a.stable[b] = n;
    }
    if (TIMED && a.tstable) {  // (uniform)
        __syncthreads();
        const int n = tsd_common_prefix<true>(tok, frm, N, nA, shortest, &s_first);
        if (threadIdx.x == 0) a.tstable[b] = n;
    }
}

__global__ __launch_bounds__(256) void tsd_stream_results_kernel(const MultiBeamArgs m) { tsd_stream_results_body<false>(m); }
__global__ __launch_bounds__(256) void tsd_stream_results_timed_kernel(const MultiBeamArgs m) { tsd_stream_results_body<true>(m); }

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct TsdStreamLayout {
    MultiBeamLayout m;
    size_t base, frm, w1, b1, total;
};

// timed: the token and frame rows together are 8 S K N words, and that count must stay below 2^31
static bool make_tsd_stream_layout(int Tc, int S, int K, int E, int N, int H, int J, int V, int joint_dtype, bool timed,
                                   TsdStreamLayout &L) {
    if (S < 1 || H < 1 || H > kTsdMaxWidth) return false;
    if (!make_multibeam_layout(Tc, S, K, E, N, J, V, joint_dtype, L.m)) return false;
    if (timed && 8ull * S * K * N >= (1ull << 31)) return false;
    const size_t R = (size_t)S * 2 * K;
    L.base = L.m.b.total;
    L.frm = align_up(L.base + (size_t)S * sizeof(int), 256);
    L.w1 = timed ? align_up(L.frm + 2 * R * (size_t)N * sizeof(int), 256) : L.frm;
    L.b1 = align_up(L.w1 + (size_t)H * J * sizeof(float), 256);
    L.total = align_up(L.b1 + (size_t)J * sizeof(float), 256);
    return true;
}

// the kernels' arguments over the workspace.  H = 1 serves step and results: what they reach lies ahead of W1
static bool tsd_stream_bind(MultiBeamArgs &m, int Tc, int S, int K, int E, int N, int H, int J, int V, int joint_dtype, bool timed,
                            void *workspace, TsdStreamLayout &L) {
    if (!make_tsd_stream_layout(Tc, S, K, E, N, H, J, V, joint_dtype, timed, L)) return false;
    MultiBeamLayout M;
    if (!multibeam_bind(m, Tc, S, K, E, N, J, V, joint_dtype, workspace, M)) return false;
    char *ws = (char *)workspace;
    m.frame_base = (const int *)(ws + L.base);
    m.frm = timed ? (int *)(ws + L.frm) : nullptr;
    return true;
}

hipError_t tsd_stream_workspace_bytes(int Tc, int S, int K, int E, int N, int H, int J, int V, int joint_dtype, bool timed,
                                      size_t *bytes) {
    TsdStreamLayout L;
    if (!make_tsd_stream_layout(Tc, S, K, E, N, H, J, V, joint_dtype, timed, L)) return hipErrorInvalidValue;
    *bytes = L.total;
    return hipSuccess;
}

hipError_t launch_tsd_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2, int H, int J, int V, int S,
                                   int Tc, int K, int E, int N, int joint_dtype, bool timed, void *workspace, hipStream_t s) {
    MultiBeamArgs m = {};
    TsdStreamLayout L;
    if (!tsd_stream_bind(m, Tc, S, K, E, N, H, J, V, joint_dtype, timed, workspace, L)) return hipErrorInvalidValue;
    const GreedyArgs &g = m.b.g;
    const int DT = L.m.b.DT;
    hipError_t e;
    if ((e = launch_greedy_w2(g, DT, W2, b2, s)) != hipSuccess) return e;
    char *ws = (char *)workspace;
    e = launch_greedy_stream_pack(W1, b1, (float *)(ws + L.w1), (float *)(ws + L.b1), H, J, g.st, S, DT == 2 ? b2 : nullptr, g.btab, V,
                                  s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tsd_stream_begin_kernel, dim3((m.b.R + 255) / 256), dim3(256), 0, s, m, (int *)(ws + L.base));
    return hipGetLastError();
}

hipError_t launch_tsd_stream_feed(const float *enc, int Te, const int *chunk_frames, const int *reset, const int *final_, int H, int J,
                                  int V, int S, int Tc, int K, int E, int N, int joint_dtype, bool timed, void *workspace,
                                  hipStream_t s) {
    MultiBeamArgs m = {};
    TsdStreamLayout L;
    if (Te < 0 || Te > Tc || !tsd_stream_bind(m, Tc, S, K, E, N, H, J, V, joint_dtype, timed, workspace, L))
        return hipErrorInvalidValue;
    const BeamArgs &b = m.b;
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
    hipLaunchKernelGGL(tsd_stream_feed_kernel, dim3(rows > 1 ? (rows < 2048 ? rows : 2048) : 1), dim3(256), 0, s, a, b.slot, b.nslot,
                       m.nclosed, K);
    return hipGetLastError();
}

template <int DT>
static hipError_t launch_tsd_stream_step_dt(const BeamArgs &a, size_t shm, hipStream_t s) {
    const hipError_t e = set_lds(tsd_stream_step_kernel<DT>, shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tsd_stream_step_kernel<DT>, dim3(a.g.NS, (a.R + 31) / 32), dim3(kGrWaves * 64), shm, s, a);
    return hipGetLastError();
}

hipError_t launch_tsd_stream_step(const float *pred_proj, int *parents, int *emitted, int J, int V, int S, int Tc, int K, int E, int N,
                                  int blank, int joint_dtype, bool timed, void *workspace, hipStream_t s) {
    MultiBeamArgs m = {};
    TsdStreamLayout L;
    if (!tsd_stream_bind(m, Tc, S, K, E, N, 1, J, V, joint_dtype, timed, workspace, L)) return hipErrorInvalidValue;
    BeamArgs &a = m.b;
    a.g.pred_proj = pred_proj, a.g.blank = blank;
    a.parents = parents, a.emitted = emitted;
    hipError_t e;
    const int DT = L.m.b.DT;
    const size_t shm = (size_t)J * 32 * sizeof(gf16) * (DT == 1 ? 1 : 2);
    if (DT == 1) e = launch_tsd_stream_step_dt<1>(a, shm, s);
    else if (DT == 0) e = launch_tsd_stream_step_dt<0>(a, shm, s);
    else e = launch_tsd_stream_step_dt<2>(a, shm, s);
    if (e != hipSuccess) return e;
    if (timed) hipLaunchKernelGGL(tsd_stream_select_timed_kernel, dim3(S), dim3(256), 0, s, m);
    else hipLaunchKernelGGL(tsd_stream_select_kernel, dim3(S), dim3(256), 0, s, m);
    return hipGetLastError();
}

hipError_t launch_tsd_stream_results(int *hyps, int *hyp_lengths, float *scores, int *stable_lengths, int *hyp_frames,
                                     int *timed_stable_lengths, int J, int V, int S, int Tc, int K, int E, int N, int joint_dtype,
                                     bool timed, void *workspace, hipStream_t s) {
    MultiBeamArgs m = {};
    TsdStreamLayout L;
    if (!tsd_stream_bind(m, Tc, S, K, E, N, 1, J, V, joint_dtype, timed, workspace, L)) return hipErrorInvalidValue;
    BeamArgs &a = m.b;
    a.hyps = hyps, a.hyp_lengths = hyp_lengths, a.scores = scores, a.stable = stable_lengths;
    a.hyp_frames = hyp_frames, a.tstable = timed_stable_lengths;
    if (timed) hipLaunchKernelGGL(tsd_stream_results_timed_kernel, dim3(S), dim3(256), 0, s, m);
    else hipLaunchKernelGGL(tsd_stream_results_kernel, dim3(S), dim3(256), 0, s, m);
    return hipGetLastError();
}

}  // namespace rnnt
