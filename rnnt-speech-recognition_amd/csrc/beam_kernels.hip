// beam_kernels.hip -- batched "modified" beam search (one symbol per frame, the k2 / icefall form) for every utterance of a batch.
//
// The beam of utterance b holds up to K hypotheses, rows b K + k of every per-hypothesis array.  Per decode step (= frame t_b of
// every utterance that has one left), for every hypothesis of the beam:
//   step    (beam_step_kernel<DT>)  the joint of greedy_step_kernel (rnnt_decode.h: the same h, operand images, MFMA chains, K
//           order and epilogue, so every logit is bitwise that of compute_rnnt_joint_logits for the hypothesis alone) over tiles
//           of 32 hypothesis rows; row r reads enc frame t_b of utterance b = r / K.  Epilogue per (vocabulary slice, row): the
//           top-K (logit, symbol) list (logit descending, symbol ascending; NaN and -inf take no part) and greedy's (max, sum of
//           exps).  Nothing of size [rows x V] is written.
//   select  (beam_select_kernel)  one workgroup per utterance: the slice lists -> per-hypothesis top-K and logsumexp (f32 partial
//           sums per chunk combined in float64, as greedy_update_kernel), the K x K candidates s_i + (logit - lse_i) ranked in
//           float64 (score descending, then hypothesis, then symbol), the first K taken, identical sequences merged (logaddexp;
//           the first-ranked survives), the new beam stably sorted by score.  Token rows are double-buffered [2][B][K][maxT] and
//           gathered by parent; two sequences are compared by (length, 64-bit rolling hash) and confirmed on the token rows.
// prepare (launch_greedy_prepare, then beam_begin_kernel): greedy's tables and W2 image, its per-utterance state (t, Tb: the
// frame counter), and every beam reset to the empty sequence with score 0.
//
// Token rows have stride N (BeamArgs::N) and the double-buffer side is GreedyState::n & 1, n = the steps the beam has taken since
// it was last reset.  Offline N = maxT and n == t.  The stream (beam_stream_*, at the end) keeps a beam across feeds: there t
// counts the frames of the current chunk, N is the token capacity of a stream, n goes on counting, and a hypothesis that holds N
// tokens offers only its blank candidate.
//
// The timed route (compute_rnnt_beam_timed_* / _stream_timed_*: beam_select_timed_kernel, beam_results_timed_kernel) keeps, beside
// the token rows, a double-buffered row of {frame, log-probability} pairs per hypothesis (BeamArgs::tt, one 8-byte element per
// token), gathered by parent exactly as the tokens are; an emission appends {n, logit - lse of the taken candidate}.  A merge
// keeps the first-ranked survivor's row.  The workspace is the untimed one with the pair rows appended.
#include "rnnt_decode.h"

namespace rnnt {
constexpr int kBeamMax = 16;
constexpr unsigned long long kHashMul = 0x9E3779B97F4A7C15ull;  // rolling hash of a prefix: h' = h kHashMul + (v + 1)
}  // namespace rnnt

#include "beam_common.h"

namespace rnnt {



// ---------------------------------------------------------------------------------------------
// prepare: every beam = [((), 0)]
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void beam_begin_kernel(const BeamArgs a) {
    for (int r = blockIdx.x * 256 + threadIdx.x; r < a.R; r += gridDim.x * 256) {
        BeamSlot s;
        s.score = (r % a.K == 0) ? 0.0 : -INFINITY;
        s.hash = 0, s.len = 0, s.pad = 0;
        a.slot[r] = s;
        if (r % a.K == 0) a.nslot[r / a.K] = 1;
    }
}

// ---------------------------------------------------------------------------------------------
// step: grid (NS vocabulary slices, ceil(B K / 32) row tiles), 4 waves; the same LDS image as greedy_step_kernel plus the
// tile's logits of the slice, [32 rows][128 symbols] (+1 padding column)
// ---------------------------------------------------------------------------------------------
#define BEAM_STEP_KERNEL beam_step_kernel
#define BEAM_STEP_BIAS 0
#include "beam_step_body.h"
#undef BEAM_STEP_KERNEL
#undef BEAM_STEP_BIAS

// ---------------------------------------------------------------------------------------------
// select: one workgroup (256 threads) per utterance
// ---------------------------------------------------------------------------------------------

#define BEAM_SELECT_KERNEL beam_select_kernel
#define BEAM_SELECT_TIMED 0
#define BEAM_SELECT_BIAS 0
#include "beam_select_body.h"
#undef BEAM_SELECT_KERNEL
#undef BEAM_SELECT_TIMED
#define BEAM_SELECT_KERNEL beam_select_timed_kernel
#define BEAM_SELECT_TIMED 1
#include "beam_select_body.h"
#undef BEAM_SELECT_KERNEL
#undef BEAM_SELECT_TIMED
#undef BEAM_SELECT_BIAS

// ---------------------------------------------------------------------------------------------
// results: one workgroup per utterance; the current beams, zero-padded; stable (NULL: not written): the length of the longest
// common prefix of the occupied hypotheses (rows 1 ... nb-1 against row 0, position by position; an integer minimum in LDS)
// ---------------------------------------------------------------------------------------------
// FR: positions agree only when the emission frames agree too (the timed stable length)
template <bool FR>
__device__ __forceinline__ int bm_common_prefix(const int *tok, const int2 *tt, const int T, const int nb, const int shortest,
                                                int *s_first) {
    if (threadIdx.x == 0) *s_first = shortest;
    __syncthreads();
    int first = shortest;
    for (int p = threadIdx.x; p < shortest && first == shortest; p += 256)
        for (int k = 1; k < nb; ++k)
            if (tok[(size_t)k * T + p] != tok[p] || (FR && tt[(size_t)k * T + p].x != tt[p].x)) first = p;
    if (first < shortest) atomicMin(s_first, first);
    __syncthreads();
    return *s_first;
}

template <bool TIMED>
__device__ __forceinline__ void beam_results_body(const BeamArgs a) {
    __shared__ int s_first;
    const GreedyArgs &g = a.g;
    const int b = blockIdx.x, K = a.K, T = a.N;
    const int cur = g.st[b].n & 1, nb = min(max(a.nslot[b], 0), K);
    const int *tok = a.tok + ((size_t)cur * g.B + b) * K * T;
    int shortest = nb > 0 ? INT_MAX : 0;
    for (int k = 0; k < K; ++k) {
        const int n = k < nb ? min(max(a.slot[b * K + k].len, 0), T) : 0;
        if (k < nb) shortest = min(shortest, n);
        for (int p = threadIdx.x; p < T; p += 256) a.hyps[((size_t)b * K + k) * T + p] = p < n ? tok[(size_t)k * T + p] : 0;
        if (TIMED) {
            const int2 *tt = a.tt + (((size_t)cur * g.B + b) * K + k) * T;
            for (int p = threadIdx.x; p < T; p += 256) {
                const int2 e = p < n ? tt[p] : make_int2(-1, 0);
                a.hyp_frames[((size_t)b * K + k) * T + p] = e.x;
                a.hyp_logp[((size_t)b * K + k) * T + p] = __int_as_float(e.y);
            }
        }
        if (threadIdx.x == 0) {
            a.hyp_lengths[b * K + k] = n;
            a.scores[b * K + k] = k < nb ? (float)a.slot[b * K + k].score : -INFINITY;
        }
    }
    if (a.stable) {  // (uniform)
        const int n = bm_common_prefix<false>(tok, nullptr, T, nb, shortest, &s_first);
        if (threadIdx.x == 0) a.stable[b] = n;
    }
    if (TIMED && a.tstable) {  // (uniform)
        __syncthreads();
        const int n = bm_common_prefix<true>(tok, a.tt + ((size_t)cur * g.B + b) * K * T, T, nb, shortest, &s_first);
        if (threadIdx.x == 0) a.tstable[b] = n;
    }
}

__global__ __launch_bounds__(256) void beam_results_kernel(const BeamArgs a) { beam_results_body<false>(a); }
__global__ __launch_bounds__(256) void beam_results_timed_kernel(const BeamArgs a) { beam_results_body<true>(a); }

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------

hipError_t beam_workspace_bytes(int T, int B, int K, int J, int V, int joint_dtype, bool timed, size_t *bytes) {
    BeamLayout L;
    if (!make_beam_layout(T, B, K, T, J, V, joint_dtype, timed, L)) return hipErrorInvalidValue;
    *bytes = L.total;
    return hipSuccess;
}

hipError_t launch_beam_begin(const float *enc_proj, const int *frame_lengths, const float *W2, const float *b2, int J, int V, int B,
                             int T, int K, int joint_dtype, bool timed, void *workspace, hipStream_t s) {
    BeamArgs a = {};
    BeamLayout L;
    if (!beam_bind(a, T, B, K, T, J, V, joint_dtype, timed, workspace, L)) return hipErrorInvalidValue;
    a.g.enc_proj = enc_proj, a.g.frame_lengths = frame_lengths, a.g.max_symbols = nullptr, a.g.max_per_frame = 0;
    hipError_t e = launch_greedy_prepare(a.g, L.DT, W2, b2, s);
    if (e != hipSuccess) return e;
    const int grid = (a.R + 255) / 256;
    hipLaunchKernelGGL(beam_begin_kernel, dim3(grid < 256 ? grid : 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

template <int DT>
static hipError_t launch_beam_step_dt(const BeamArgs &a, size_t shm, hipStream_t s) {
    const hipError_t e = set_lds(beam_step_kernel<DT>, shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(beam_step_kernel<DT>, dim3(a.g.NS, (a.R + 31) / 32), dim3(kGrWaves * 64), shm, s, a);
    return hipGetLastError();
}

// N: the token row stride the workspace was laid out with (offline: T; the stream: max_hyp_len)
hipError_t launch_beam_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits, int *topk_symbols, float *lse,
                            int J, int V, int B, int T, int K, int N, int blank, int joint_dtype, bool timed, void *workspace,
                            hipStream_t s) {
    BeamArgs a = {};
    BeamLayout L;
    if (!beam_bind(a, T, B, K, N, J, V, joint_dtype, timed, workspace, L)) return hipErrorInvalidValue;
    a.g.pred_proj = pred_proj, a.g.blank = blank;
    a.parents = parents, a.emitted = emitted, a.topl = topk_logits, a.tops = topk_symbols, a.lse = lse;
    hipError_t e;
    const size_t shm = (size_t)J * 32 * sizeof(gf16) * (L.DT == 1 ? 1 : 2);
    if (L.DT == 1) e = launch_beam_step_dt<1>(a, shm, s);
    else if (L.DT == 0) e = launch_beam_step_dt<0>(a, shm, s);
    else e = launch_beam_step_dt<2>(a, shm, s);
    if (e != hipSuccess) return e;
    if (timed) hipLaunchKernelGGL(beam_select_timed_kernel, dim3(B), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(beam_select_kernel, dim3(B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// hyp_frames != NULL: the timed results (hyp_logp too; timed_stable_lengths or NULL) of a workspace laid out timed
hipError_t launch_beam_results(int *hyps, int *hyp_lengths, float *scores, int *stable_lengths, int *hyp_frames, float *hyp_logp,
                               int *timed_stable_lengths, int J, int V, int B, int T, int K, int N, int joint_dtype, void *workspace,
                               hipStream_t s) {
    BeamArgs a = {};
    BeamLayout L;
    const bool timed = hyp_frames != nullptr;
    if (!beam_bind(a, T, B, K, N, J, V, joint_dtype, timed, workspace, L)) return hipErrorInvalidValue;
    a.hyps = hyps, a.hyp_lengths = hyp_lengths, a.scores = scores, a.stable = stable_lengths;
    a.hyp_frames = hyp_frames, a.hyp_logp = hyp_logp, a.tstable = timed_stable_lengths;
    if (timed) hipLaunchKernelGGL(beam_results_timed_kernel, dim3(B), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(beam_results_kernel, dim3(B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// stream: beam search over a stream of chunks per slot (include/rnnt.h compute_rnnt_beam_stream_*).  The workspace is the beam
// workspace with T = max_chunk_frames, B = slots and token rows of stride N = max_hyp_len, then W1 [H][J] and b1 [J] as the
// greedy stream lays them out: beam_step_kernel, beam_select_kernel and beam_results_kernel run on it unchanged.  A feed refills
// the tables for the chunk's frames (greedy_stream_proj_kernel: the one FMA chain the chunking equivalence rests on) and sets
// every slot's frame cursor; GreedyState::n (the step count) and the beam live on until a reset.
// ---------------------------------------------------------------------------------------------
// begin: every beam empty (the slots' states were set finished by launch_greedy_stream_pack)
__global__ __launch_bounds__(256) void beam_stream_begin_kernel(const BeamArgs a) {
    for (int r = blockIdx.x * 256 + threadIdx.x; r < a.R; r += gridDim.x * 256) {
        BeamSlot s;
        s.score = -INFINITY, s.hash = 0, s.len = 0, s.pad = 0;
        a.slot[r] = s;
        if (r % a.K == 0) a.nslot[r / a.K] = 0;
    }
}

// the per-frame range flags of the chunk's frames (as greedy_stream_feed_kernel forms them); workgroup 0 also moves every slot on
__global__ __launch_bounds__(256) void beam_stream_feed_kernel(const GreedyStreamArgs a, BeamSlot *slot, int *nslot, const int K) {
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
        if (a.reset && a.reset[b] != 0) {  // a new stream: the beam [((), 0)], no steps taken
            s.n = 0, s.fin = 0;
            for (int k = 0; k < K; ++k) {
                BeamSlot e;
                e.score = k == 0 ? 0.0 : -INFINITY, e.hash = 0, e.len = 0, e.pad = 0;
                slot[b * K + k] = e;
            }
            nslot[b] = 1;
        }
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

static bool make_beam_stream_layout(int Tc, int S, int K, int N, int H, int J, int V, int joint_dtype, bool timed, BeamLayout &L,
                                    size_t &w1, size_t &b1) {
    if (S < 1 || K < 1 || K > kBeamMax || (long long)S * K > 1024 || H < 1 || H > 4096) return false;  // (the prediction network's rows)
    if (!make_beam_layout(Tc, S, K, N, J, V, joint_dtype, timed, L)) return false;
    w1 = L.total;
    b1 = align_up(w1 + (size_t)H * J * sizeof(float), 256);
    L.total = align_up(b1 + (size_t)J * sizeof(float), 256);
    return true;
}

hipError_t beam_stream_workspace_bytes(int Tc, int S, int K, int N, int H, int J, int V, int joint_dtype, bool timed, size_t *bytes) {
    BeamLayout L;
    size_t w1, b1;
    if (!make_beam_stream_layout(Tc, S, K, N, H, J, V, joint_dtype, timed, L, w1, b1)) return hipErrorInvalidValue;
    *bytes = L.total;
    return hipSuccess;
}

hipError_t launch_beam_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2, int H, int J, int V, int S,
                                    int Tc, int K, int N, int joint_dtype, bool timed, void *workspace, hipStream_t s) {
    BeamLayout L;
    size_t w1, bo;
    if (!make_beam_stream_layout(Tc, S, K, N, H, J, V, joint_dtype, timed, L, w1, bo)) return hipErrorInvalidValue;
    BeamArgs a = {};
    if (!beam_bind(a, Tc, S, K, N, J, V, joint_dtype, timed, workspace, L)) return hipErrorInvalidValue;
    hipError_t e;
    if ((e = launch_greedy_w2(a.g, L.DT, W2, b2, s)) != hipSuccess) return e;
    char *ws = (char *)workspace;
    e = launch_greedy_stream_pack(W1, b1, (float *)(ws + w1), (float *)(ws + bo), H, J, a.g.st, S, L.DT == 2 ? b2 : nullptr, a.g.btab,
                                  V, s);
    if (e != hipSuccess) return e;
    const int grid = (a.R + 255) / 256;
    hipLaunchKernelGGL(beam_stream_begin_kernel, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_beam_stream_feed(const float *enc, int Te, const int *chunk_frames, const int *reset, const int *final_, int H, int J,
                                   int V, int S, int Tc, int K, int N, int joint_dtype, bool timed, void *workspace, hipStream_t s) {
    BeamLayout L;
    size_t w1, bo;
    if (!make_beam_stream_layout(Tc, S, K, N, H, J, V, joint_dtype, timed, L, w1, bo) || Te < 0 || Te > Tc) return hipErrorInvalidValue;
    BeamArgs b = {};
    if (!beam_bind(b, Tc, S, K, N, J, V, joint_dtype, timed, workspace, L)) return hipErrorInvalidValue;
    char *ws = (char *)workspace;
    GreedyStreamArgs a = {};
    a.enc = enc, a.W1 = (const float *)(ws + w1), a.b1 = (const float *)(ws + bo);
    a.chunk_frames = chunk_frames, a.reset = reset, a.final_ = final_;
    a.st = b.g.st, a.rowflag = b.g.rowflag, a.expE = b.g.expE, a.encraw = b.g.encraw;
    a.S = S, a.Te = Te, a.T = Tc, a.H = H, a.J = J;
    const hipError_t e = launch_greedy_stream_proj(a, s);
    if (e != hipSuccess) return e;
    const int rows = S * Te;
    hipLaunchKernelGGL(beam_stream_feed_kernel, dim3(rows > 1 ? (rows < 2048 ? rows : 2048) : 1), dim3(256), 0, s, a, b.slot, b.nslot,
                       K);
    return hipGetLastError();
}

}  // namespace rnnt
