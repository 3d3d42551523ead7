// beam_select_body.h -- the select kernel of beam_kernels.hip, included there once per instantiation: BEAM_SELECT_KERNEL is the
// kernel's name and BEAM_SELECT_TIMED 0 / 1 whether it keeps the {frame, log-probability} rows (beam_select_kernel and
// beam_select_timed_kernel).  One source, kernels with names of their own: all are compiled as kernels, so the untimed one
// comes out of the compiler as it did before the timed one existed.  No include guard on purpose.
// BEAM_SELECT_BIAS 1 (beam_select_bias_kernel, beam_select_timed_bias_kernel): the context graph bg.  The slice lists hold raw
// logits in key order; beta and the next state of every listed entry are re-derived by bisection (s_pb / s_pn, the entries
// spread over the wave's lanes), the lists are merged on the key logit + beta, beta goes into the candidate's score in float64
// and the next state travels with the candidate into BeamSlot::pad.  Everything of it is compiled out at 0.
// BEAM_SELECT_BIAS 2 (beam_select_lm_kernel, beam_select_timed_lm_kernel): bg is the n-gram LM of include/rnnt_lm.h (LmArgs), with
// bg_state / bg_delta overloads of its own (beam_lm_kernels.hip); the body is the biased one.
#if BEAM_SELECT_BIAS
#if BEAM_SELECT_BIAS == 2
__global__ __launch_bounds__(256) void BEAM_SELECT_KERNEL(const BeamArgs a, const LmArgs bg) {
#else
__global__ __launch_bounds__(256) void BEAM_SELECT_KERNEL(const BeamArgs a, const BiasArgs bg) {
#endif
    __shared__ float s_pb[kGrWaves][64 * kBeamMax], s_tb[kBeamMax * kBeamMax];
    __shared__ int s_pn[kGrWaves][64 * kBeamMax], s_tn[kBeamMax * kBeamMax], s_q[kBeamMax], s_nx[kBeamMax];
#else
__global__ __launch_bounds__(256) void BEAM_SELECT_KERNEL(const BeamArgs a) {
#endif
    constexpr bool TIMED = BEAM_SELECT_TIMED;
    __shared__ float s_tl[kBeamMax * kBeamMax];  // per-hypothesis top-K
    __shared__ int s_tv[kBeamMax * kBeamMax];
    __shared__ double s_lse[kBeamMax], s_cs[kBeamMax * kBeamMax], s_term[kGrWaves][64];
    __shared__ int s_rank[kBeamMax * kBeamMax], s_take[kBeamMax];
    __shared__ int s_len[kBeamMax], s_par[kBeamMax], s_v[kBeamMax], s_same[kBeamMax * kBeamMax], s_ord[kBeamMax];
    __shared__ unsigned long long s_hash[kBeamMax];
    __shared__ double s_sc[kBeamMax];
    __shared__ int s_m, s_n;
    const GreedyArgs &g = a.g;
    const int b = blockIdx.x, K = a.K, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, blank = g.blank;
    const GreedyState st = g.st[b];
    const int rb = b * K;
    if (st.t >= st.Tb) {  // frozen: nothing changes
        if (tid < K) a.parents[rb + tid] = rb + tid, a.emitted[rb + tid] = -1;
#if BEAM_SELECT_BIAS
        if (tid < K && bg.states) bg.states[rb + tid] = a.slot[rb + tid].pad;
#endif
        return;
    }
    const int nb = a.nslot[b], T = a.N, cur = st.n & 1;
    const int *tok_cur = a.tok + ((size_t)cur * g.B + b) * K * T;
    int *tok_nxt = a.tok + ((size_t)(cur ^ 1) * g.B + b) * K * T;

    // ---- per hypothesis (one wave each): logsumexp as greedy_update_kernel, the slice lists merged into the top-K
    for (int i = wave; i < nb; i += kGrWaves) {
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
            for (int q = 0; q < g.NS; ++q) S += s_term[wave][q];  // slice order, as greedy_update_kernel
            s_lse[i] = (double)M + log(S);
            if (a.lse) a.lse[r] = (float)s_lse[i];
        }
#if BEAM_SELECT_BIAS
        const int qi = bg_state(bg, a.slot[r].pad);
        if (lane == 0) s_q[i] = qi;
        for (int e = lane; e < g.NS * K; e += 64) {  // entry e % K of slice e / K
            const int v = a.pv[((size_t)(e / K) * a.R + r) * K + e % K];
            int nx = qi;
            const float be = v >= 0 ? bg_delta(bg, qi, v, blank, nx) : 0.f;
            s_pb[wave][e] = be, s_pn[wave][e] = nx;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
        int h = 0;
        for (int k = 0; k < K; ++k) {
            float l = -INFINITY;
            int v = INT_MAX;
#if BEAM_SELECT_BIAS
            float raw = -INFINITY;
            if (lane < g.NS && h < K) {
                const size_t o = ((size_t)lane * a.R + r) * K + h;
                if (a.pv[o] >= 0) raw = a.pl[o], v = a.pv[o], l = raw + s_pb[wave][lane * K + h];  // (the step's key)
            }
#else
            if (lane < g.NS && h < K) {
                const size_t o = ((size_t)lane * a.R + r) * K + h;
                if (a.pv[o] >= 0) l = a.pl[o], v = a.pv[o];
            }
#endif
            const int mine = v;
            float bl = l;
            int bv = v;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const float ol = __shfl_xor(bl, off);
                const int ov = __shfl_xor(bv, off);
                if (bm_better(ol, ov, bl, bv)) bl = ol, bv = ov;
            }
#if BEAM_SELECT_BIAS
            if (bv != INT_MAX ? bv == mine : lane == 0) {  // the winning lane: the raw logit, beta and the next state
                s_tl[i * K + k] = bv != INT_MAX ? raw : -INFINITY;
                s_tv[i * K + k] = bv != INT_MAX ? bv : -1;
                s_tb[i * K + k] = bv != INT_MAX ? s_pb[wave][lane * K + h] : 0.f;
                s_tn[i * K + k] = bv != INT_MAX ? s_pn[wave][lane * K + h] : qi;
                if (a.topl) a.topl[(size_t)r * K + k] = bv != INT_MAX ? raw : -INFINITY;
                if (a.tops) a.tops[(size_t)r * K + k] = bv != INT_MAX ? bv : -1;
            }
            if (bv != INT_MAX && bv == mine) ++h;
#else
            if (bv != INT_MAX && bv == mine) ++h;
            if (lane == 0) {
                s_tl[i * K + k] = bv != INT_MAX ? bl : -INFINITY;
                s_tv[i * K + k] = bv != INT_MAX ? bv : -1;
                if (a.topl) a.topl[(size_t)r * K + k] = bv != INT_MAX ? bl : -INFINITY;
                if (a.tops) a.tops[(size_t)r * K + k] = bv != INT_MAX ? bv : -1;
            }
#endif
        }
    }
    __syncthreads();
    // a hypothesis whose token row is full (N tokens; never offline) offers its blank candidate alone
    if (tid < nb && a.slot[rb + tid].len >= a.N) {
        for (int k = 0; k < K; ++k) s_tv[tid * K + k] = -1;
        s_tv[tid * K] = blank, s_tl[tid * K] = a.bl[rb + tid];
#if BEAM_SELECT_BIAS
        s_tb[tid * K] = 0.f, s_tn[tid * K] = s_q[tid];
#endif
    }
    __syncthreads();

    // ---- the nb K candidates in float64, ranked by (score desc, hypothesis asc, symbol asc); NaN / -inf never taken
    const int nc = nb * K;
    if (tid < nc) {
        const int i = tid / K;
#if BEAM_SELECT_BIAS
        const double sc = a.slot[rb + i].score + ((double)s_tl[tid] - s_lse[i]) + (double)s_tb[tid];
#else
        const double sc = a.slot[rb + i].score + ((double)s_tl[tid] - s_lse[i]);
#endif
        s_cs[tid] = (s_tv[tid] >= 0 && sc > -INFINITY) ? sc : __builtin_nan("");
    }
    if (tid == 0) s_m = 0;
    __syncthreads();
    if (tid < nc) {
        const double sc = s_cs[tid];
        int rank = -1;
        if (sc == sc) {
            rank = 0;
            for (int c = 0; c < nc; ++c) {
                const double o = s_cs[c];
                if (o > sc || (o == sc && (c / K < tid / K || (c / K == tid / K && s_tv[c] < s_tv[tid])))) ++rank;
            }
        }
        if (rank >= 0 && rank < K) s_take[rank] = tid, atomicAdd(&s_m, 1);
    }
    __syncthreads();
    const int m = s_m;

    // ---- the taken candidates' sequences: y_i, or y_i + (v,)
    if (tid < m) {
        const int c = s_take[tid], i = c / K, v = s_tv[c];
        const BeamSlot p = a.slot[rb + i];
        const bool emit = v != blank;
        s_par[tid] = i, s_v[tid] = emit ? v : -1;
        s_len[tid] = p.len + (emit ? 1 : 0);
        s_hash[tid] = emit ? p.hash * kHashMul + (unsigned long long)(v + 1) : p.hash;
        s_sc[tid] = s_cs[c];
#if BEAM_SELECT_BIAS
        s_nx[tid] = s_tn[c];
#endif
    } else if (m == 0 && tid < nb) {  // nothing can be taken: the beam is carried over unchanged
        const BeamSlot p = a.slot[rb + tid];
#if BEAM_SELECT_BIAS
        s_nx[tid] = p.pad;
#endif
        s_par[tid] = tid, s_v[tid] = -1, s_len[tid] = p.len, s_hash[tid] = p.hash, s_sc[tid] = p.score;
    }
    __syncthreads();
    const int nt = m > 0 ? m : nb;
    // same (length, hash): confirmed on the token rows before a merge
    if (tid < kBeamMax * kBeamMax) {
        const int x = tid / kBeamMax, y = tid % kBeamMax;
        s_same[tid] = (m > 0 && x < y && y < m && s_len[x] == s_len[y] && s_hash[x] == s_hash[y]) ? 1 : 0;
    }
    __syncthreads();
    for (int x = 0; x < m; ++x)
        for (int y = x + 1; y < m; ++y) {
            if (!s_same[x * kBeamMax + y]) continue;  // (LDS, uniform)
            const int *rx = tok_cur + (size_t)s_par[x] * T, *ry = tok_cur + (size_t)s_par[y] * T;
            const int lx = a.slot[rb + s_par[x]].len, ly = a.slot[rb + s_par[y]].len;
            bool diff = false;
            for (int p = tid; p < s_len[x]; p += 256)
                diff |= bm_token(rx, lx, s_v[x], p) != bm_token(ry, ly, s_v[y], p);
            diff = __syncthreads_or(diff);
            if (tid == 0 && diff) s_same[x * kBeamMax + y] = 0;
        }
    __syncthreads();
    // merge (the first-ranked survives, logaddexp in float64), then a stable sort by score, descending
    if (tid == 0) {
        int alive = 0;
        for (int x = 0; x < nt; ++x) {
            if (s_sc[x] != s_sc[x]) continue;  // (merged away below)
            for (int y = x + 1; y < nt; ++y)
                if (s_same[x * kBeamMax + y] && s_sc[y] == s_sc[y]) {
                    const double hi = fmax(s_sc[x], s_sc[y]), lo2 = fmin(s_sc[x], s_sc[y]);
                    s_sc[x] = hi + log1p(exp(lo2 - hi));
                    s_sc[y] = __builtin_nan("");
                }
            int p = alive++;
            while (p > 0 && s_sc[s_ord[p - 1]] < s_sc[x]) s_ord[p] = s_ord[p - 1], --p;
            s_ord[p] = x;
        }
        s_n = alive;
    }
    __syncthreads();
    const int nn = s_n;
    // ---- the new beam: slots, parents, emitted, token rows gathered by parent
    if (tid < K) {
        const int r = rb + tid;
        BeamSlot s;
        s.pad = 0;
        if (tid < nn) {
            const int x = s_ord[tid];
            s.score = s_sc[x], s.hash = s_hash[x], s.len = s_len[x];
#if BEAM_SELECT_BIAS
            s.pad = s_nx[x];  // (identical sequences have identical states: a merge keeps the survivor's)
#endif
            a.parents[r] = rb + s_par[x], a.emitted[r] = s_v[x];
        } else {
            s.score = -INFINITY, s.hash = 0, s.len = 0;
            a.parents[r] = r, a.emitted[r] = -1;
        }
        a.slot[r] = s;
#if BEAM_SELECT_BIAS
        if (bg.states) bg.states[r] = s.pad;
#endif
    }
    for (int k = 0; k < nn; ++k) {
        const int x = s_ord[k], i = s_par[x], n = s_len[x];
        const int li = n - (s_v[x] >= 0 ? 1 : 0);
        for (int p = tid; p < n; p += 256) tok_nxt[(size_t)k * T + p] = bm_token(tok_cur + (size_t)i * T, li, s_v[x], p);
        if (TIMED) {  // the pair row of the parent; an emission appends this frame and the taken candidate's logit - lse
            const int2 *tt_cur = a.tt + (((size_t)cur * g.B + b) * K + i) * T;
            int2 *tt_nxt = a.tt + (((size_t)(cur ^ 1) * g.B + b) * K + k) * T;
            int lp = 0;
            if (li < n) {  // (an emission: m > 0, x is a taken candidate)
                const int c = s_take[x];
                lp = __float_as_int((float)((double)s_tl[c] - s_lse[c / K]));
            }
            // (the pair as two scalars, selected per element and packed at the store: an int2 variable that is modified and then
            // selected whole ends up in scratch)
            for (int p = tid; p < n; p += 256) {
                int ef = st.n, el = lp;
                if (p < li) ef = tt_cur[p].x, el = tt_cur[p].y;
                tt_nxt[p] = make_int2(ef, el);
            }
        }
    }
    if (tid == 0) {
        a.nslot[b] = nn;
        GreedyState s2 = st;
        s2.t = st.t + 1, s2.n = st.n + 1;
        g.st[b] = s2;
    }
}
