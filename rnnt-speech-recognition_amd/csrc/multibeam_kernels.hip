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
#include "rnnt_decode.h"

namespace rnnt {
constexpr int kBeamMax = 16;
constexpr unsigned long long kHashMul = 0x9E3779B97F4A7C15ull;  // beam_kernels.hip's: h' = h kHashMul + (v + 1)
}  // namespace rnnt

#include "beam_common.h"

namespace rnnt {

struct MultiBeamArgs {
    BeamArgs b;  // K = beam, R = minibatch 2 K rows, N = max_hyp_len; nslot = |A|; slot / tok / parents / emitted over the 2 K rows
    int *nclosed;  // [B] |B|
    int E;         // symbols per frame
};

// ---------------------------------------------------------------------------------------------
// the workspace: BeamLayout's regions over R = B 2K rows (lists of K per row), and |B| per utterance
// ---------------------------------------------------------------------------------------------
struct MultiBeamLayout {
    BeamLayout b;
    size_t nclosed;
};

static bool make_multibeam_layout(int T, int B, int K, int E, int N, int J, int V, int joint_dtype, MultiBeamLayout &M) {
    BeamLayout &L = M.b;
    L.DT = greedy_dt(joint_dtype, J, V);
    if (L.DT < 0 || T <= 0 || B <= 0 || K < 1 || K > kBeamMax || N < 1 || E < 1 || E > 8) return false;
    if ((long long)B * 2 * K > 1024) return false;  // (the prediction network's rows)
    if ((unsigned long long)B * T * J >= (1ull << 31) || 4ull * B * K * N >= (1ull << 31)) return false;
    if ((unsigned long long)T * (E + 1) >= (1ull << 31)) return false;  // (the step counter)
    L.NC = (V + 31) / 32;
    L.NS = (L.NC + kGrWaves - 1) / kGrWaves;
    const size_t R = (size_t)B * 2 * K;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    L.st = take((size_t)B * sizeof(GreedyState));
    L.slot = take(R * sizeof(BeamSlot));
    L.nslot = take((size_t)B * sizeof(int));
    M.nclosed = take((size_t)B * sizeof(int));
    L.pm = take((size_t)L.NS * R * sizeof(float));
    L.ps = take((size_t)L.NS * R * sizeof(float));
    L.pl = take((size_t)L.NS * R * K * sizeof(float));
    L.pv = take((size_t)L.NS * R * K * sizeof(int));
    L.tok = take(2 * R * (size_t)N * sizeof(int));
    L.rowflag = take((size_t)B * T * sizeof(int));
    L.expE = take((size_t)B * T * J * sizeof(float));
    L.encraw = take((size_t)B * T * J * sizeof(float));
    L.img = take(L.DT == 1 ? (size_t)L.NC * 32 * J * sizeof(gf16) : joint_w2_image_bytes(J, V));
    L.btab = take((size_t)L.NC * 32 * sizeof(float));
    L.tflag = take(256 + 1024);  // joint_prep_kernel's flag words + b2s (as greedy's layout)
    L.bl = take(R * sizeof(float));
    L.tt = off;
    L.total = off;
    return true;
}

static bool multibeam_bind(MultiBeamArgs &m, int T, int B, int K, int E, int N, int J, int V, int joint_dtype, void *workspace,
                           MultiBeamLayout &M) {
    if (!make_multibeam_layout(T, B, K, E, N, J, V, joint_dtype, M)) return false;
    const BeamLayout &L = M.b;
    char *ws = (char *)workspace;
    BeamArgs &a = m.b;
    GreedyArgs &g = a.g;
    g.st = (GreedyState *)(ws + L.st);
    g.part_m = (float *)(ws + L.pm), g.part_s = (float *)(ws + L.ps);
    g.rowflag = (int *)(ws + L.rowflag);
    g.expE = (float *)(ws + L.expE), g.encraw = (float *)(ws + L.encraw);
    g.img = (gf16 *)(ws + L.img), g.btab = (float *)(ws + L.btab), g.tflag = (const float *)(ws + L.tflag);
    g.NC = L.NC, g.NS = L.NS;
    g.B = B, g.T = T, g.J = J, g.V = V;
    a.slot = (BeamSlot *)(ws + L.slot), a.nslot = (int *)(ws + L.nslot);
    a.pl = (float *)(ws + L.pl), a.pv = (int *)(ws + L.pv), a.bl = (float *)(ws + L.bl), a.tok = (int *)(ws + L.tok);
    a.tt = nullptr;
    a.K = K, a.R = B * 2 * K, a.N = N;
    m.nclosed = (int *)(ws + M.nclosed);
    m.E = E;
    return true;
}

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
__global__ __launch_bounds__(256) void multibeam_select_kernel(const MultiBeamArgs m) {
    constexpr int KM = kBeamMax;
    __shared__ float s_tl[KM * KM];  // per open hypothesis: its top-K non-blank logits
    __shared__ int s_tv[KM * KM];    // and their symbols (-1: none)
    __shared__ double s_lse[KM], s_cs[KM * KM], s_term[kGrWaves][64];
    __shared__ int s_take[KM];
    // the 2 K slots as the step found them: [0, K) the open list, [K, 2K) the closed list
    __shared__ double s_sc[2 * KM];
    __shared__ unsigned long long s_hash[2 * KM];
    __shared__ int s_len[2 * KM];
    __shared__ double s_cl[KM];       // the closings c_i (NaN: skipped)
    __shared__ int s_same[KM * KM];   // [i][j]: open i and closed j hold the same sequence
    // the closed list of this round before the sort: the old entries in their order, then the fresh closings in A's order
    __shared__ double s_lsc[2 * KM];
    __shared__ int s_lsrc[2 * KM];    // the slot (0 .. 2K-1) that holds the entry's sequence and state
    __shared__ int s_ord[2 * KM];     // the sorted list: entry of rank k
    __shared__ int s_nl;
    const BeamArgs &a = m.b;
    const GreedyArgs &g = a.g;
    const int b = blockIdx.x, K = a.K, KR = 2 * K, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, blank = g.blank;
    const GreedyState st = g.st[b];
    const int rb = b * KR;
    if (st.t >= st.Tb) {  // frozen: nothing changes
        if (tid < KR) a.parents[rb + tid] = rb + tid, a.emitted[rb + tid] = -1;
        return;
    }
    const int N = a.N, cur = st.n & 1, round = st.nf;
    const int nA = min(max(a.nslot[b], 0), K), nB = min(max(m.nclosed[b], 0), K);
    const int *tok_cur = a.tok + ((size_t)cur * g.B + b) * KR * N;
    int *tok_nxt = a.tok + ((size_t)(cur ^ 1) * g.B + b) * KR * N;
    if (tid < KR) {
        const bool used = tid < K ? tid < nA : tid - K < nB;
        BeamSlot p;
        p.score = -INFINITY, p.hash = 0, p.len = 0;
        if (used) p = a.slot[rb + tid];
        s_sc[tid] = p.score, s_hash[tid] = p.hash, s_len[tid] = min(max(p.len, 0), N);
    }

    // ---- per open hypothesis (one wave each): logsumexp as beam_select_kernel, the slice lists merged into the top-K
    for (int i = wave; i < nA; i += kGrWaves) {
        const int r = rb + i;
        const float pm = lane < g.NS ? g.part_m[(size_t)lane * a.R + r] : -INFINITY;
        const float ps = lane < g.NS ? g.part_s[(size_t)lane * a.R + r] : 0.f;
        float M = pm;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float o = __shfl_xor(M, off);
            if (o > M) M = o;
        }
        s_term[wave][lane] = ps > 0.f ? (double)ps * exp((double)pm - (double)M) : 0.0;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (one wave: its LDS operations complete in order)
        if (lane == 0) {
            double S = 0.0;
            for (int q = 0; q < g.NS; ++q) S += s_term[wave][q];  // slice order, as beam_select_kernel
            s_lse[i] = (double)M + log(S);
        }
        int h = 0;
        for (int k = 0; k < K; ++k) {
            float l = -INFINITY;
            int v = INT_MAX;
            if (lane < g.NS && h < K) {
                const size_t o = ((size_t)lane * a.R + r) * K + h;
                if (a.pv[o] >= 0) l = a.pl[o], v = a.pv[o];
            }
            const int mine = v;
            float bl = l;
            int bv = v;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const float ol = __shfl_xor(bl, off);
                const int ov = __shfl_xor(bv, off);
                if (bm_better(ol, ov, bl, bv)) bl = ol, bv = ov;
            }
            if (bv != INT_MAX && bv == mine) ++h;
            if (lane == 0) {
                s_tl[i * K + k] = bv != INT_MAX ? bl : -INFINITY;
                s_tv[i * K + k] = bv != INT_MAX ? bv : -1;
            }
        }
    }
    __syncthreads();

    // ---- closings: c_i = s_i + lp_i(blank); NaN and -inf are skipped
    if (tid < K) {
        double c = __builtin_nan("");
        if (tid < nA) {
            c = s_sc[tid] + ((double)a.bl[rb + tid] - s_lse[tid]);
            if (!(c > -INFINITY)) c = __builtin_nan("");
        }
        s_cl[tid] = c;
    }
    __syncthreads();
    // open i against closed j: the same (length, hash), confirmed on the token rows below
    {
        const int i = tid / KM, j = tid % KM;
        s_same[tid] = (i < nA && j < nB && s_cl[i] == s_cl[i] && s_len[i] == s_len[K + j] && s_hash[i] == s_hash[K + j]) ? 1 : 0;
    }
    __syncthreads();
    for (int i = 0; i < nA; ++i)
        for (int j = 0; j < nB; ++j) {
            if (!s_same[i * KM + j]) continue;  // (LDS, uniform)
            const int *ri = tok_cur + (size_t)i * N, *rj = tok_cur + (size_t)(K + j) * N;
            bool diff = false;
            for (int p = tid; p < s_len[i]; p += 256) diff |= ri[p] != rj[p];
            diff = __syncthreads_or(diff);
            if (tid == 0 && diff) s_same[i * KM + j] = 0;
        }
    __syncthreads();
    // the list: old entries keep their places (a closing of the same sequence is added in, logaddexp in float64), fresh ones are
    // appended in A's order.  Two open hypotheses never share a sequence, so an entry takes at most one closing per round.
    if (tid == 0) {
        int n = nB;
        for (int j = 0; j < nB; ++j) s_lsc[j] = s_sc[K + j], s_lsrc[j] = K + j;
        for (int i = 0; i < nA; ++i) {
            const double c = s_cl[i];
            if (c != c) continue;
            int hit = -1;
            for (int j = 0; j < nB && hit < 0; ++j)
                if (s_same[i * KM + j]) hit = j;
            if (hit >= 0) {
                const double hi = fmax(s_lsc[hit], c), lo = fmin(s_lsc[hit], c);
                s_lsc[hit] = hi + log1p(exp(lo - hi));
            } else {
                s_lsc[n] = c, s_lsrc[n] = i, ++n;
            }
        }
        s_nl = n;
    }
    __syncthreads();
    const int nl = s_nl;  // <= 2 K
    if (tid < nl) {       // the stable sort by score, descending: rank by counting
        const double sc = s_lsc[tid];
        int rank = 0;
        for (int c = 0; c < nl; ++c) {
            const double o = s_lsc[c];
            if (o > sc || (o == sc && c < tid)) ++rank;
        }
        s_ord[rank] = tid;
    }
    const int nB2 = min(nl, K);

    // ---- expansions (rounds r < E): the nA K candidates in float64, ranked by (score desc, hypothesis asc, symbol asc)
    const bool expand = round < m.E;
    const int nc = expand ? nA * K : 0;
    bool valid = false;
    if (tid < nc) {
        const int i = tid / K;
        const double sc = s_sc[i] + ((double)s_tl[tid] - s_lse[i]);
        valid = s_tv[tid] >= 0 && s_len[i] < N && sc > -INFINITY;
        s_cs[tid] = valid ? sc : __builtin_nan("");
    }
    const int mA = min(__syncthreads_count(valid), K);  // (also: s_cs and s_ord are visible)
    if (valid) {
        const double sc = s_cs[tid];
        int rank = 0;
        for (int c = 0; c < nc; ++c) {
            const double o = s_cs[c];
            if (o > sc || (o == sc && (c / K < tid / K || (c / K == tid / K && s_tv[c] < s_tv[tid])))) ++rank;
        }
        if (rank < K) s_take[rank] = tid;
    }
    __syncthreads();

    // ---- the new lists: slots, parents, emitted (all parents name rows as they were before this step)
    const bool turn = !expand;  // round E: A := B, B := []
    if (tid < KR) {
        const int r = rb + tid;
        BeamSlot s;
        s.score = -INFINITY, s.hash = 0, s.len = 0, s.pad = 0;
        int par = r, em = -1;
        if (tid < K) {
            if (turn) {
                if (tid < nB2) {
                    const int e = s_ord[tid], src = s_lsrc[e];
                    s.score = s_lsc[e], s.hash = s_hash[src], s.len = s_len[src], par = rb + src;
                }
            } else if (tid < mA) {
                const int c = s_take[tid], i = c / K, v = s_tv[c];
                s.score = s_cs[c], s.hash = s_hash[i] * kHashMul + (unsigned long long)(v + 1), s.len = s_len[i] + 1;
                par = rb + i, em = v;
            }
        } else if (!turn && tid - K < nB2) {
            const int e = s_ord[tid - K], src = s_lsrc[e];
            s.score = s_lsc[e], s.hash = s_hash[src], s.len = s_len[src], par = rb + src;
        }
        a.slot[r] = s;
        a.parents[r] = par, a.emitted[r] = em;
    }
    // token rows, gathered by parent: the sorted closed list (into B's rows, at the turn into A's), the expansions into A's
    for (int k = 0; k < nB2; ++k) {
        const int src = s_lsrc[s_ord[k]], n = s_len[src];
        int *dst = tok_nxt + (size_t)(turn ? k : K + k) * N;
        for (int p = tid; p < n; p += 256) dst[p] = tok_cur[(size_t)src * N + p];
    }
    if (!turn)
        for (int k = 0; k < mA; ++k) {
            const int c = s_take[k], i = c / K, n = s_len[i];
            int *dst = tok_nxt + (size_t)k * N;
            for (int p = tid; p < n; p += 256) dst[p] = tok_cur[(size_t)i * N + p];
            if (tid == 0) dst[n] = s_tv[c];  // (n < N: a hypothesis of N tokens offers no expansion)
        }
    if (tid == 0) {
        a.nslot[b] = turn ? nB2 : mA;
        m.nclosed[b] = turn ? 0 : nB2;
        GreedyState s2 = st;
        s2.n = st.n + 1;
        if (turn) s2.t = st.t + 1, s2.nf = 0;
        else s2.nf = round + 1;
        g.st[b] = s2;
    }
}

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
