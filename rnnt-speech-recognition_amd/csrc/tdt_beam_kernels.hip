// tdt_beam_kernels.hip -- batched beam search of a token-and-duration (TDT) transducer (include/rnnt_tdt_beam.h): the frame-synchronous,
// one-symbol-per-frame search of beam_kernels.hip on the TDT rule.  The joint has R = V + D columns: V token logits, then D duration
// logits.  A hypothesis is (token sequence, cursor, score); the cursor is the next frame it reads.  Per decode step (= frame t of
// every utterance that has one left):
//   step    (tdt_beam_step_kernel<DT>)  beam_step_kernel's grid over tiles of 32 hypothesis rows and NS slices of the R columns, for
//           the ACTIVE rows alone (slot occupied, t < T_b, cursor == t): a waiting hypothesis costs no joint.  The joint is
//           rnnt_decode.h's, unchanged.  The epilogue keeps TWO (max, sum of exps) pairs per lane, as tdt_greedy_step_kernel does:
//           columns v < V feed the token pair, columns V <= v < R the duration pair, padding neither; both heads' partials are
//           written per (slice, row), the empty partial (-inf, 0) where a slice holds no column of a head.  The slice's top-K list is
//           beam_step_body.h's over the token columns alone (duration and padding columns enter the LDS tile as NaN).  The up to D
//           raw duration logits of a row go to dl [rows][8] from whichever slice(s) hold them.
//   select  (tdt_beam_select_kernel / _timed_kernel)  one workgroup per utterance, float64.  Per active hypothesis: both logsumexps
//           (slice order, as tdt_greedy_update_kernel), the slice lists merged into the token top-K, the K D (token, duration) pairs
//           scored and the best K of them kept under the key (score, v, j).  A waiting hypothesis offers its `stay`.  Then
//           beam_select_kernel's tail with the cursor in it: rank by counting under (score desc, hypothesis, stay / v, j), take K,
//           find duplicates on (length, rolling hash, cursor) confirmed on the token rows, merge (logaddexp, the first-ranked
//           survives), stable sort, write slots, parents, emitted and the double-buffered token rows; timed: the {frame, duration}
//           rows beside them.
// prepare  launch_greedy_prepare at alphabet_size = R, then tdt_beam_begin_kernel: every beam = [((), 0, 0)] and the duration set,
//           which arrives as kernel arguments.
// Workspace: tdt_beam_common.h.  The step kernel and the select body live in tdt_beam_step_body.h and tdt_beam_select_body.h, which
// tdt_nbest_stream_kernels.hip (the stream over slots) compiles a second time with its stream flag on; here the flag is off.
#include "rnnt_decode.h"

namespace rnnt {
constexpr int kBeamMax = 16;
constexpr unsigned long long kHashMul = 0x9E3779B97F4A7C15ull;  // beam_kernels.hip's: h' = h kHashMul + (v + 1)
}  // namespace rnnt

#include "tdt_beam_common.h"

namespace rnnt {

// ---------------------------------------------------------------------------------------------
// prepare: every beam = [((), cursor 0, score 0)]; the duration set
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tdt_beam_begin_kernel(const TdtBeamArgs ta, const TdtBeamDurations dur) {
    const BeamArgs &a = ta.b;
    if (blockIdx.x == 0 && threadIdx.x < kTdtBeamMaxD) ta.durset[threadIdx.x] = dur.d[threadIdx.x];
    for (int r = blockIdx.x * 256 + threadIdx.x; r < a.R; r += gridDim.x * 256) {
        BeamSlot s;
        s.score = (r % a.K == 0) ? 0.0 : -INFINITY;
        s.hash = 0, s.len = 0, s.pad = 0;
        a.slot[r] = s;
        if (r % a.K == 0) a.nslot[r / a.K] = 1;
    }
}

// ---------------------------------------------------------------------------------------------
// step: grid (NS slices of the R columns, ceil(B K / 32) row tiles), 4 waves; beam_step_kernel's LDS
// ---------------------------------------------------------------------------------------------
#define TDT_BEAM_STEP_KERNEL tdt_beam_step_kernel
#define TDT_BEAM_STEP_STREAM 0
#include "tdt_beam_step_body.h"
#undef TDT_BEAM_STEP_KERNEL
#undef TDT_BEAM_STEP_STREAM

// ---------------------------------------------------------------------------------------------
// select: one workgroup (256 threads) per utterance
// ---------------------------------------------------------------------------------------------
#include "tdt_beam_select_body.h"

__global__ __launch_bounds__(256) void tdt_beam_select_kernel(const TdtBeamArgs ta) { tdt_beam_select_body<false, false>(ta); }
__global__ __launch_bounds__(256) void tdt_beam_select_timed_kernel(const TdtBeamArgs ta) { tdt_beam_select_body<true, false>(ta); }

// ---------------------------------------------------------------------------------------------
// results: one workgroup per utterance; the current beams, best first
// ---------------------------------------------------------------------------------------------
template <bool TIMED>
__device__ __forceinline__ void tdt_beam_results_body(const TdtBeamArgs &ta) {
    const BeamArgs &a = ta.b;
    const GreedyArgs &g = a.g;
    const int b = blockIdx.x, K = a.K, T = a.N;
    const int cur = g.st[b].n & 1, nb = min(max(a.nslot[b], 0), K);
    const int *tok = a.tok + ((size_t)cur * g.B + b) * K * T;
    for (int k = 0; k < K; ++k) {
        const int n = k < nb ? min(max(a.slot[b * K + k].len, 0), T) : 0;
        for (int p = threadIdx.x; p < T; p += 256) a.hyps[((size_t)b * K + k) * T + p] = p < n ? tok[(size_t)k * T + p] : 0;
        if (TIMED) {
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
            if (ta.cursors) ta.cursors[b * K + k] = k < nb ? a.slot[b * K + k].pad : -1;
        }
    }
}

__global__ __launch_bounds__(256) void tdt_beam_results_kernel(const TdtBeamArgs ta) { tdt_beam_results_body<false>(ta); }
__global__ __launch_bounds__(256) void tdt_beam_results_timed_kernel(const TdtBeamArgs ta) { tdt_beam_results_body<true>(ta); }

// ---------------------------------------------------------------------------------------------
// host side (the layout and its binding: tdt_beam_common.h)
// ---------------------------------------------------------------------------------------------
hipError_t tdt_beam_workspace_bytes(int T, int B, int K, int J, int Vt, int D, int joint_dtype, bool timed, size_t *bytes) {
    TdtBeamLayout L;
    if (!make_tdt_beam_layout(T, B, K, J, Vt, D, joint_dtype, timed, L)) return hipErrorInvalidValue;
    *bytes = L.total;
    return hipSuccess;
}

hipError_t launch_tdt_beam_begin(const float *enc_proj, const int *frame_lengths, const float *W2, const float *b2, int J, int Vt,
                                 const int *durations, int D, int B, int T, int K, int joint_dtype, bool timed, void *workspace,
                                 hipStream_t s) {
    TdtBeamArgs ta = {};
    TdtBeamLayout L;
    if (!tdt_beam_bind(ta, T, B, K, J, Vt, D, joint_dtype, timed, workspace, L)) return hipErrorInvalidValue;
    GreedyArgs &g = ta.b.g;
    g.enc_proj = enc_proj, g.frame_lengths = frame_lengths, g.max_symbols = nullptr, g.max_per_frame = 0;
    const hipError_t e = launch_greedy_prepare(g, L.b.DT, W2, b2, s);
    if (e != hipSuccess) return e;
    TdtBeamDurations dur;
    for (int i = 0; i < kTdtBeamMaxD; ++i) dur.d[i] = i < D ? durations[i] : 0;
    const int grid = (ta.b.R + 255) / 256;
    hipLaunchKernelGGL(tdt_beam_begin_kernel, dim3(grid < 256 ? grid : 256), dim3(256), 0, s, ta, dur);
    return hipGetLastError();
}

template <int DT>
static hipError_t launch_tdt_beam_step_dt(const TdtBeamArgs &ta, size_t shm, hipStream_t s) {
    const hipError_t e = set_lds(tdt_beam_step_kernel<DT>, shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tdt_beam_step_kernel<DT>, dim3(ta.b.g.NS, (ta.b.R + 31) / 32), dim3(kGrWaves * 64), shm, s, ta);
    return hipGetLastError();
}

hipError_t launch_tdt_beam_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits, int *topk_symbols,
                                float *dur_logits, float *lse, int J, int Vt, int D, int B, int T, int K, int blank, int joint_dtype,
                                bool timed, void *workspace, hipStream_t s) {
    TdtBeamArgs ta = {};
    TdtBeamLayout L;
    if (!tdt_beam_bind(ta, T, B, K, J, Vt, D, joint_dtype, timed, workspace, L)) return hipErrorInvalidValue;
    BeamArgs &a = ta.b;
    a.g.pred_proj = pred_proj, a.g.blank = blank;
    a.parents = parents, a.emitted = emitted, a.topl = topk_logits, a.tops = topk_symbols, a.lse = lse;
    ta.durl = dur_logits;
    hipError_t e;
    const size_t shm = (size_t)J * 32 * sizeof(gf16) * (L.b.DT == 1 ? 1 : 2);
    if (L.b.DT == 1) e = launch_tdt_beam_step_dt<1>(ta, shm, s);
    else if (L.b.DT == 0) e = launch_tdt_beam_step_dt<0>(ta, shm, s);
    else e = launch_tdt_beam_step_dt<2>(ta, shm, s);
    if (e != hipSuccess) return e;
    if (timed) hipLaunchKernelGGL(tdt_beam_select_timed_kernel, dim3(B), dim3(256), 0, s, ta);
    else hipLaunchKernelGGL(tdt_beam_select_kernel, dim3(B), dim3(256), 0, s, ta);
    return hipGetLastError();
}

// hyp_frames != NULL: the timed results (hyp_durations too) of a workspace laid out timed
hipError_t launch_tdt_beam_results(int *hyps, int *hyp_lengths, float *scores, int *cursors, int *hyp_frames, int *hyp_durations,
                                   int J, int Vt, int D, int B, int T, int K, int joint_dtype, bool timed, void *workspace,
                                   hipStream_t s) {
    TdtBeamArgs ta = {};
    TdtBeamLayout L;
    if (!tdt_beam_bind(ta, T, B, K, J, Vt, D, joint_dtype, timed, workspace, L)) return hipErrorInvalidValue;
    BeamArgs &a = ta.b;
    a.hyps = hyps, a.hyp_lengths = hyp_lengths, a.scores = scores, a.hyp_frames = hyp_frames;
    ta.cursors = cursors, ta.hyp_durations = hyp_durations;
    if (hyp_frames) hipLaunchKernelGGL(tdt_beam_results_timed_kernel, dim3(B), dim3(256), 0, s, ta);
    else hipLaunchKernelGGL(tdt_beam_results_kernel, dim3(B), dim3(256), 0, s, ta);
    return hipGetLastError();
}

}  // namespace rnnt
