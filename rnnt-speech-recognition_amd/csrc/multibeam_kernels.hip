// multibeam_kernels.hip -- batched beam search with several symbols per frame (include/rnnt_beam_multi.h: the time-synchronous
// search on the STANDARD lattice, where beam_kernels.hip is the one-symbol-per-frame "modified" search).
//
// Utterance b owns 2 K rows of every per-hypothesis array: rows b 2K + k (k < K) are the OPEN list A, rows b 2K + K + k the CLOSED
// list B.  One decode step is one ROUND r of one frame t of every utterance that has a frame left (GreedyState: t the frame, nf
// the round, n the steps taken = the side of the double-buffered token rows):
//   step    (multibeam_step_kernel<DT>)  beam_step_body.h at its flag value 3: beam_step_kernel's grid, tiling, joint and MFMA
//           chains (rnnt_decode.h, unchanged) over tiles of 32 rows, 2 K rows per utterance of which the first nslot[b] (A) are
//           live.  Per (slice, live row): the top-K list over the NON-BLANK symbols, greedy's (max, sum of exps), and from the
//           slice that holds it the blank's logit.  A tile without live rows reads and writes nothing.
//   select  (multibeam_select_kernel)  one workgroup per utterance, float64: per open hypothesis the logsumexp (slice order, as
//           beam_select_kernel) and the slice lists merged into its top-K; the CLOSINGS s_i + lp_i(blank) merged into B on the
//           sequence ((length, rolling hash) confirmed on the token rows), B stably sorted and cut to K; in rounds r < E the
//           EXPANSIONS ranked by counting under (score desc, hypothesis, symbol) and the first K made the new A; in round r = E
//           the frame turn A := B, B := [].  parents / emitted for all 2 K rows, the slots, the token rows gathered by parent.
// begin   launch_greedy_prepare (tables, W2 image, per-utterance state), then multibeam_begin_kernel: A = [((), 0)], B = [].
// results multibeam_results_kernel: list A, best first.
// No atomics, no memset; every word of the workspace that is read was written since begin.
// The argument block, the layout and the bind are in multibeam_common.h and the select kernel's body in multibeam_select_body.h:
// tsd_stream_kernels.hip (the stream of include/rnnt_beam_multi_stream.h) compiles the same text under names of its own.
#include "rnnt_decode.h"

namespace rnnt {
constexpr int kBeamMax = 16;
constexpr unsigned long long kHashMul = 0x9E3779B97F4A7C15ull;  // beam_kernels.hip's: h' = h kHashMul + (v + 1)
}  // namespace rnnt

#include "multibeam_common.h"

namespace rnnt {

// ---------------------------------------------------------------------------------------------
// begin: A = [((), 0)], B = []
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void multibeam_begin_kernel(const MultiBeamArgs m) {
    const BeamArgs &a = m.b;
    const int KR = 2 * a.K;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < a.R; r += gridDim.x * 256) {
        BeamSlot s;
        s.score = (r % KR == 0) ? 0.0 : -INFINITY;
        s.hash = 0, s.len = 0, s.pad = 0;
        a.slot[r] = s;
        if (r % KR == 0) a.nslot[r / KR] = 1, m.nclosed[r / KR] = 0;
    }
}

// ---------------------------------------------------------------------------------------------
// step: grid (NS vocabulary slices, ceil(B 2K / 32) row tiles), 4 waves; beam_step_kernel's LDS
// ---------------------------------------------------------------------------------------------
#define BEAM_STEP_KERNEL multibeam_step_kernel
#define BEAM_STEP_BIAS 3
#include "beam_step_body.h"
#undef BEAM_STEP_KERNEL
#undef BEAM_STEP_BIAS

// ---------------------------------------------------------------------------------------------
// select: one workgroup (256 threads) per utterance
// ---------------------------------------------------------------------------------------------
#include "multibeam_select_body.h"

__global__ __launch_bounds__(256) void multibeam_select_kernel(const MultiBeamArgs m) { multibeam_select_body<false>(m); }

// ---------------------------------------------------------------------------------------------
// results: one workgroup per utterance; list A, best first, zero-padded
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void multibeam_results_kernel(const MultiBeamArgs m) {
    const BeamArgs &a = m.b;
    const GreedyArgs &g = a.g;
    const int b = blockIdx.x, K = a.K, KR = 2 * K, N = a.N;
    const int cur = g.st[b].n & 1, nA = min(max(a.nslot[b], 0), K);
    const int *tok = a.tok + ((size_t)cur * g.B + b) * KR * N;
    for (int k = 0; k < K; ++k) {
        const int n = k < nA ? min(max(a.slot[b * KR + k].len, 0), N) : 0;
        for (int p = threadIdx.x; p < N; p += 256) a.hyps[((size_t)b * K + k) * N + p] = p < n ? tok[(size_t)k * N + p] : 0;
        if (threadIdx.x == 0) {
            a.hyp_lengths[b * K + k] = n;
            a.scores[b * K + k] = k < nA ? (float)a.slot[b * KR + k].score : -INFINITY;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
hipError_t multibeam_workspace_bytes(int T, int B, int K, int E, int N, int J, int V, int joint_dtype, size_t *bytes) {
    MultiBeamLayout M;
    if (!make_multibeam_layout(T, B, K, E, N, J, V, joint_dtype, M)) return hipErrorInvalidValue;
    *bytes = M.b.total;
    return hipSuccess;
}

hipError_t launch_multibeam_begin(const float *enc_proj, const int *frame_lengths, const float *W2, const float *b2, int J, int V,
                                  int B, int T, int K, int E, int N, int joint_dtype, void *workspace, hipStream_t s) {
    MultiBeamArgs m = {};
    MultiBeamLayout M;
    if (!multibeam_bind(m, T, B, K, E, N, J, V, joint_dtype, workspace, M)) return hipErrorInvalidValue;
    GreedyArgs &g = m.b.g;
    g.enc_proj = enc_proj, g.frame_lengths = frame_lengths, g.max_symbols = nullptr, g.max_per_frame = 0;
    const hipError_t e = launch_greedy_prepare(g, M.b.DT, W2, b2, s);
    if (e != hipSuccess) return e;
    const int grid = (m.b.R + 255) / 256;
    hipLaunchKernelGGL(multibeam_begin_kernel, dim3(grid), dim3(256), 0, s, m);
    return hipGetLastError();
}

template <int DT>
static hipError_t launch_multibeam_step_dt(const BeamArgs &a, size_t shm, hipStream_t s) {
    const hipError_t e = set_lds(multibeam_step_kernel<DT>, shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(multibeam_step_kernel<DT>, dim3(a.g.NS, (a.R + 31) / 32), dim3(kGrWaves * 64), shm, s, a);
    return hipGetLastError();
}

hipError_t launch_multibeam_step(const float *pred_proj, int *parents, int *emitted, int J, int V, int B, int T, int K, int E, int N,
                                 int blank, int joint_dtype, void *workspace, hipStream_t s) {
    MultiBeamArgs m = {};
    MultiBeamLayout M;
    if (!multibeam_bind(m, T, B, K, E, N, J, V, joint_dtype, workspace, M)) return hipErrorInvalidValue;
    BeamArgs &a = m.b;
    a.g.pred_proj = pred_proj, a.g.blank = blank;
    a.parents = parents, a.emitted = emitted;
    hipError_t e;
    const size_t shm = (size_t)J * 32 * sizeof(gf16) * (M.b.DT == 1 ? 1 : 2);
    if (M.b.DT == 1) e = launch_multibeam_step_dt<1>(a, shm, s);
    else if (M.b.DT == 0) e = launch_multibeam_step_dt<0>(a, shm, s);
    else e = launch_multibeam_step_dt<2>(a, shm, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(multibeam_select_kernel, dim3(B), dim3(256), 0, s, m);
    return hipGetLastError();
}

hipError_t launch_multibeam_results(int *hyps, int *hyp_lengths, float *scores, int J, int V, int B, int T, int K, int E, int N,
                                    int joint_dtype, void *workspace, hipStream_t s) {
    MultiBeamArgs m = {};
    MultiBeamLayout M;
    if (!multibeam_bind(m, T, B, K, E, N, J, V, joint_dtype, workspace, M)) return hipErrorInvalidValue;
    m.b.hyps = hyps, m.b.hyp_lengths = hyp_lengths, m.b.scores = scores;
    hipLaunchKernelGGL(multibeam_results_kernel, dim3(B), dim3(256), 0, s, m);
    return hipGetLastError();
}

}  // namespace rnnt
