// multibeam_select_body.h -- the select kernel of the beam search with several symbols per frame, shared by multibeam_kernels.hip
// (TIMED false) and tsd_stream_kernels.hip (TIMED false and true: the stream of include/rnnt_beam_multi_stream.h, whose timed form
// keeps per token the frame that appended it in MultiBeamArgs::frm, gathered by parent exactly as the token rows).  The includer
// has included multibeam_common.h.  What the kernel does: the head of multibeam_kernels.hip.
#pragma once

template <bool TIMED>
__device__ __forceinline__ void multibeam_select_body(const MultiBeamArgs &m) {
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
        if (TIMED) {  // an entry a closing was added into keeps ITS OWN frame row, as it keeps its state
            const int *fsrc = m.frm + (((size_t)cur * g.B + b) * KR + src) * N;
            int *fdst = m.frm + (((size_t)(cur ^ 1) * g.B + b) * KR + (turn ? k : K + k)) * N;
            for (int p = tid; p < n; p += 256) fdst[p] = fsrc[p];
        }
    }
    if (!turn)
        for (int k = 0; k < mA; ++k) {
            const int c = s_take[k], i = c / K, n = s_len[i];
            int *dst = tok_nxt + (size_t)k * N;
            for (int p = tid; p < n; p += 256) dst[p] = tok_cur[(size_t)i * N + p];
            if (tid == 0) dst[n] = s_tv[c];  // (n < N: a hypothesis of N tokens offers no expansion)
            if (TIMED) {  // the parent's frames, then the frame of this evaluation, counted from the slot's reset
                const int *fsrc = m.frm + (((size_t)cur * g.B + b) * KR + i) * N;
                int *fdst = m.frm + (((size_t)(cur ^ 1) * g.B + b) * KR + k) * N;
                for (int p = tid; p < n; p += 256) fdst[p] = fsrc[p];
                if (tid == 0) fdst[n] = m.frame_base[b] + st.t;
            }
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
