// tdt_beam_select_body.h -- the select kernel of the TDT beam searches, shared by tdt_beam_kernels.hip (STREAM false) and
// tdt_nbest_stream_kernels.hip (STREAM true: the full-row rule of include/rnnt_tdt_beam_stream.h, and timed rows that hold the frame
// since the slot's reset).  The token and pair rows have stride BeamArgs::N on both routes.  The includer has included
// tdt_beam_common.h.  What the kernel does: the head of tdt_beam_kernels.hip.
#pragma once

// the head's logsumexp of row r from its NS partials, by one wave: the maximum by shuffles, the terms in float64 into term[64]
__device__ __forceinline__ float tb_head_terms(const float *pm_, const float *ps_, const int NS, const int R, const int r, const int lane,
                                               double *term) {
    const float pm = lane < NS ? pm_[(size_t)lane * R + r] : -INFINITY;
    const float ps = lane < NS ? ps_[(size_t)lane * R + r] : 0.f;
    float M = pm;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(M, off);
        if (o > M) M = o;
    }
    term[lane] = ps > 0.f ? (double)ps * exp((double)pm - (double)M) : 0.0;
    return M;
}

template <bool TIMED, bool STREAM>
__device__ __forceinline__ void tdt_beam_select_body(const TdtBeamArgs &ta) {
    const BeamArgs &a = ta.b;
    constexpr int KK = kBeamMax * kBeamMax, PW = kBeamMax * kTdtBeamMaxD;
    __shared__ float s_tl[KK], s_dlg[kBeamMax * kTdtBeamMaxD];  // per-hypothesis token top-K, duration logits
    __shared__ int s_tv[KK];
    __shared__ double s_lt[kBeamMax], s_ld[kBeamMax], s_term[kGrWaves][64], s_term2[kGrWaves][64];
    __shared__ double s_ps[kGrWaves][PW];  // a hypothesis's K D pair scores
    __shared__ double s_cs[KK];            // candidates: hypothesis i's at i K ..., in its own rank order
    __shared__ int s_cv[KK], s_cj[KK];     // their token (-1: stay) and duration index
    __shared__ int s_act[kBeamMax], s_take[kBeamMax];
    __shared__ int s_len[kBeamMax], s_par[kBeamMax], s_v[kBeamMax], s_cur[kBeamMax], s_dur[kBeamMax], s_same[KK], s_ord[kBeamMax];
    __shared__ unsigned long long s_hash[kBeamMax];
    __shared__ double s_sc[kBeamMax];
    __shared__ int s_m, s_n;
    const GreedyArgs &g = a.g;
    const int b = blockIdx.x, K = a.K, D = ta.D, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, blank = g.blank;
    const GreedyState st = g.st[b];
    const int rb = b * K;
    if (st.t >= st.Tb) {  // frozen: nothing changes
        if (tid < K) a.parents[rb + tid] = rb + tid, a.emitted[rb + tid] = -1;
        return;
    }
    const int nb = a.nslot[b], T = a.N, cur = st.n & 1, t = st.t;
    const int *tok_cur = a.tok + ((size_t)cur * g.B + b) * K * T;
    int *tok_nxt = a.tok + ((size_t)(cur ^ 1) * g.B + b) * K * T;
    if (tid < kBeamMax) s_act[tid] = tid < nb && a.slot[rb + tid].pad == t ? 1 : 0;
    if (tid == 0) s_m = 0;
    __syncthreads();

    // ---- per active hypothesis (one wave each): both logsumexps, the slice lists merged into the token top-K, the duration logits
    for (int i0 = 0; i0 < nb; i0 += kGrWaves) {  // (block-uniform trip count; `on` is wave-uniform)
        const int i = i0 + wave, r = rb + i;
        const bool on = i < nb && s_act[i];
        float MT = 0.f, MD = 0.f;
        if (on) {
            MT = tb_head_terms(g.part_m, g.part_s, g.NS, a.R, r, lane, s_term[wave]);
            MD = tb_head_terms(ta.dpart_m, ta.dpart_s, g.NS, a.R, r, lane, s_term2[wave]);
        }
        __syncthreads();
        if (on && lane == 0) {
            double S = 0.0, S2 = 0.0;
            for (int q = 0; q < g.NS; ++q) S += s_term[wave][q];  // slice order, as tdt_greedy_update_kernel
            for (int q = 0; q < g.NS; ++q) S2 += s_term2[wave][q];
            s_lt[i] = (double)MT + log(S), s_ld[i] = (double)MD + log(S2);
            if (a.lse) a.lse[2 * (size_t)r] = (float)s_lt[i], a.lse[2 * (size_t)r + 1] = (float)s_ld[i];
        }
        if (on && lane < D) {
            const float l = ta.dl[(size_t)r * kTdtBeamMaxD + lane];
            s_dlg[i * kTdtBeamMaxD + lane] = l;
            if (ta.durl) ta.durl[(size_t)r * D + lane] = l;
        }
        if (on) {
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
                    if (a.topl) a.topl[(size_t)r * K + k] = bv != INT_MAX ? bl : -INFINITY;
                    if (a.tops) a.tops[(size_t)r * K + k] = bv != INT_MAX ? bv : -1;
                }
            }
        }
        __syncthreads();
    }
    if (STREAM) {  // an active hypothesis whose token row is full (N tokens; never offline) offers its blank alone, with every duration
        if (tid < nb && s_act[tid] && a.slot[rb + tid].len >= a.N) {
            for (int k = 0; k < K; ++k) s_tv[tid * K + k] = -1;
            s_tv[tid * K] = blank, s_tl[tid * K] = a.bl[rb + tid];
        }
        __syncthreads();
    }

    // ---- per hypothesis its candidates, in its own rank order at s_cs[i K ...]: an active one the best K of its K D (token,
    // duration) pairs under (score desc, v asc, j asc), a waiting one its stay; NaN: no candidate
    for (int i0 = 0; i0 < nb; i0 += kGrWaves) {
        const int i = i0 + wave;
        const bool there = i < nb, on = there && s_act[i];
        const double si = there ? a.slot[rb + i].score : 0.0;
        if (there)
            for (int k = lane; k < K; k += 64) {
                const bool stay = !on && k == 0;
                s_cs[i * K + k] = stay ? si : __builtin_nan("");
                s_cv[i * K + k] = -1, s_cj[i * K + k] = 0;
            }
        if (on)
            for (int e = lane; e < K * D; e += 64) {
                const int k = e / D, j = e - k * D;
                const double sc = si + (((double)s_tl[i * K + k] - s_lt[i]) + ((double)s_dlg[i * kTdtBeamMaxD + j] - s_ld[i]));
                s_ps[wave][e] = (s_tv[i * K + k] >= 0 && sc > -INFINITY) ? sc : __builtin_nan("");  // (a NaN fails the comparison)
            }
        __syncthreads();
        if (on)
            for (int e = lane; e < K * D; e += 64) {
                const double sc = s_ps[wave][e];
                if (sc != sc) continue;
                const int k = e / D, j = e - k * D, v = s_tv[i * K + k];
                int rank = 0;
                for (int c = 0; c < K * D; ++c) {
                    const double o = s_ps[wave][c];
                    const int kc = c / D, jc = c - kc * D, vc = s_tv[i * K + kc];
                    if (o > sc || (o == sc && (vc < v || (vc == v && jc < j)))) ++rank;
                }
                if (rank < K) s_cs[i * K + rank] = sc, s_cv[i * K + rank] = v, s_cj[i * K + rank] = j;
            }
        __syncthreads();
    }

    // ---- the nb K candidates ranked by (score desc, hypothesis asc, then the hypothesis's own order); NaN never taken
    const int nc = nb * K;
    if (tid < nc) {
        const double sc = s_cs[tid];
        int rank = -1;
        if (sc == sc) {
            rank = 0;
            for (int c = 0; c < nc; ++c) {
                const double o = s_cs[c];
                if (o > sc || (o == sc && c < tid)) ++rank;
            }
        }
        if (rank >= 0 && rank < K) s_take[rank] = tid, atomicAdd(&s_m, 1);  // (LDS)
    }
    __syncthreads();
    const int m = s_m;

    // ---- the taken candidates' successors: (y_i, c_i) for a stay, (y_i [+ v], t + d) otherwise
    if (tid < m) {
        const int c = s_take[tid], i = c / K, v = s_cv[c];
        const BeamSlot *p = a.slot + rb + i;  // (read per field: a slot copied whole in two branches ends up in scratch)
        const bool stay = !s_act[i];
        const bool emit = !stay && v != blank;
        int d = 0;
        if (!stay) {
            d = ta.durset[s_cj[c]];
            if (d == 0) d = 1;  // one symbol per frame, and a blank must move
        }
        s_par[tid] = i, s_v[tid] = emit ? v : -1;
        const unsigned long long ph = p->hash;
        s_len[tid] = p->len + (emit ? 1 : 0);
        s_hash[tid] = emit ? ph * kHashMul + (unsigned long long)(v + 1) : ph;
        s_sc[tid] = s_cs[c];
        s_cur[tid] = stay ? p->pad : t + d, s_dur[tid] = d;
    } else if (m == 0 && tid < nb) {  // nothing can be taken: the beam is carried over, every cursor one frame on
        const BeamSlot *p = a.slot + rb + tid;
        s_par[tid] = tid, s_v[tid] = -1, s_len[tid] = p->len, s_hash[tid] = p->hash, s_sc[tid] = p->score;
        s_cur[tid] = t + 1, s_dur[tid] = 0;
    }
    __syncthreads();
    const int nt = m > 0 ? m : nb;
    // the stream: cursors count from the chunk's first frame, the timed rows from the slot's reset
    const int tbase = STREAM && TIMED ? (ta.tail + ta.durset[kTdtBeamBaseWord])[b] : 0;
    // same (length, hash, cursor): confirmed on the token rows before a merge
    if (tid < KK) {
        const int x = tid / kBeamMax, y = tid % kBeamMax;
        s_same[tid] =
            (m > 0 && x < y && y < m && s_len[x] == s_len[y] && s_hash[x] == s_hash[y] && s_cur[x] == s_cur[y]) ? 1 : 0;
    }
    __syncthreads();
    for (int x = 0; x < m; ++x)
        for (int y = x + 1; y < m; ++y) {
            if (!s_same[x * kBeamMax + y]) continue;  // (LDS, uniform)
            const int *rx = tok_cur + (size_t)s_par[x] * T, *ry = tok_cur + (size_t)s_par[y] * T;
            const int lx = a.slot[rb + s_par[x]].len, ly = a.slot[rb + s_par[y]].len;
            bool diff = false;
            for (int p = tid; p < s_len[x]; p += 256) diff |= bm_token(rx, lx, s_v[x], p) != bm_token(ry, ly, s_v[y], p);
            diff = __syncthreads_or(diff);
            if (tid == 0 && diff) s_same[x * kBeamMax + y] = 0;
        }
    __syncthreads();
    // merge (the first-ranked survives, logaddexp in float64, folded in rank order), then a stable sort by score, descending
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
    // ---- the new beam: slots (the cursor in BeamSlot::pad), parents, emitted, token rows gathered by parent
    if (tid < K) {
        const int r = rb + tid;
        const bool in = tid < nn;  // (selected per field and stored per field: a slot built in two branches ends up in scratch)
        const int x = in ? s_ord[tid] : 0;
        BeamSlot *sp = a.slot + r;
        sp->score = in ? s_sc[x] : -INFINITY, sp->hash = in ? s_hash[x] : 0ull, sp->len = in ? s_len[x] : 0, sp->pad = in ? s_cur[x] : 0;
        a.parents[r] = in ? rb + s_par[x] : r, a.emitted[r] = in ? s_v[x] : -1;
    }
    for (int k = 0; k < nn; ++k) {
        const int x = s_ord[k], i = s_par[x], n = s_len[x];
        const int li = n - (s_v[x] >= 0 ? 1 : 0);
        for (int p = tid; p < n; p += 256) tok_nxt[(size_t)k * T + p] = bm_token(tok_cur + (size_t)i * T, li, s_v[x], p);
        if (TIMED) {  // the pair row of the parent; an emission appends {this frame, the frames it claims}
            const int2 *tt_cur = a.tt + (((size_t)cur * g.B + b) * K + i) * T;
            int2 *tt_nxt = a.tt + (((size_t)(cur ^ 1) * g.B + b) * K + k) * T;
            const int d = s_dur[x];
            for (int p = tid; p < n; p += 256) {  // (two scalars, packed at the store: see beam_select_body.h)
                int ef = tbase + t, ed = d;
                if (p < li) ef = tt_cur[p].x, ed = tt_cur[p].y;
                tt_nxt[p] = make_int2(ef, ed);
            }
        }
    }
    if (tid == 0) {
        a.nslot[b] = nn;
        g.st[b].t = st.t + 1, g.st[b].n = st.n + 1;  // (the frame counter and the double-buffer side; nothing else changes)
    }
}
