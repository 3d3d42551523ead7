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
// Workspace: tdt_beam_common.h.
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

// one column into a running (max, sum) pair: the arithmetic of greedy_step_kernel's epilogue
__device__ __forceinline__ void tb_feed(const float l, float &bm, float &bs) {
    if (l > bm) {
        bs = fmaf(bs, __builtin_amdgcn_exp2f((bm - l) * kLog2e), 1.0f);
        bm = l;
    } else {
        bs += __builtin_amdgcn_exp2f((l - bm) * kLog2e);
    }
}

// the 2 kGrWaves partials of row n of the tile, in greedy_step_kernel's order -> one partial
__device__ __forceinline__ void tb_combine(const float *r_m, const float *r_s, const int n, float &M, float &S) {
    M = -INFINITY;
    for (int q = 0; q < 2 * kGrWaves; ++q) {
        const int src = (q >> 1) * 64 + n + 32 * (q & 1);
        if (r_m[src] > M) M = r_m[src];
    }
    S = 0.f;
    for (int q = 0; q < 2 * kGrWaves; ++q) {
        const int src = (q >> 1) * 64 + n + 32 * (q & 1);
        if (r_s[src] > 0.f) S += r_s[src] * __builtin_amdgcn_exp2f((r_m[src] - M) * kLog2e);
    }
}

// ---------------------------------------------------------------------------------------------
// step: grid (NS slices of the R columns, ceil(B K / 32) row tiles), 4 waves; beam_step_kernel's LDS
// ---------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(kGrWaves * 64) void tdt_beam_step_kernel(const TdtBeamArgs ta) {
    const BeamArgs &ba = ta.b;
    const GreedyArgs &a = ba.g;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_t[32], s_live[32], s_slow[32];
    __shared__ float r_m[kGrWaves * 64], r_s[kGrWaves * 64], q_m[kGrWaves * 64], q_s[kGrWaves * 64];
    __shared__ float stage[DT == 2 ? 32 * 33 : 1];
    __shared__ float lg[32 * (32 * kGrWaves + 1)];
    constexpr int LW = 32 * kGrWaves + 1;
    const int J = a.J, K = ba.K;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, n31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slice = blockIdx.x, r0 = blockIdx.y * 32;

    bool live = false;
    if (tid < 32) {
        const int r = r0 + tid, b = r / K;
        int t = 0, slow = 0;
        if (r < ba.R) {
            const GreedyState s = a.st[b];
            live = s.t < s.Tb && r - b * K < ba.nslot[b] && ba.slot[r].pad == s.t;  // active: the cursor is this frame
            t = min(max(s.t, 0), a.T - 1);
            if (live) slow = a.rowflag[(size_t)b * a.T + t];
        }
        s_live[tid] = live ? 1 : 0, s_t[tid] = t, s_slow[tid] = slow;
    }
    if (!__syncthreads_or(live)) return;  // a tile without an active hypothesis reads and writes nothing
    dec_pred_route(a, J, r0, s_live, s_slow, tid);
    __syncthreads();
    gf16 *hA = (gf16 *)smem, *hL = hA + (size_t)J * 32;
    const bool hform = DT == 0 && a.tflag[1] != 0.f;
    dec_build_h<DT>(a, J, r0, s_live, s_slow, [&](int n) { return (size_t)((r0 + n) / K) * a.T + s_t[n]; }, hform, hA, hL, tid);
    __syncthreads();

    // ---- this wave's chunk of 32 columns: tokens below Vt, durations from Vt to R, padding beyond
    const int vc = slice * kGrWaves + wave;
    float bm = -INFINITY, bs = 0.f, dm = -INFINITY, ds = 0.f;
    if (vc < a.NC) {
        const gf32x16 acc = dec_chunk_acc<DT>(a, vc, hA, hL, stage, lane);
        float m2inv, w2inv;
        dec_logit_scales<DT>(a, hform, m2inv, w2inv);
        const bool row_live = s_live[n31] != 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {  // in increasing column order
            const int vv = gr_cdrow(r, half), v = 32 * vc + vv;
            const float l = dec_logit<DT>(a, acc[r], vc, vv, v, m2inv, w2inv);
            if (v < ta.Vt) {
                tb_feed(l, bm, bs);
            } else if (v < a.V) {
                tb_feed(l, dm, ds);
                if (row_live) ta.dl[(size_t)(r0 + n31) * kTdtBeamMaxD + (v - ta.Vt)] = l;
            }
            lg[n31 * LW + 32 * wave + vv] = v < ta.Vt ? l : __builtin_nanf("");  // (the top-K below: token columns alone)
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) lg[n31 * LW + 32 * wave + gr_cdrow(r, half)] = __builtin_nanf("");
    }
    r_m[tid] = bm, r_s[tid] = bs;
    q_m[tid] = dm, q_s[tid] = ds;
    __syncthreads();
    if (tid < 32 && s_live[tid]) {  // both heads' partials of row tid
        const size_t o = (size_t)slice * ba.R + r0 + tid;
        float M, S;
        tb_combine(r_m, r_s, tid, M, S);
        a.part_m[o] = M, a.part_s[o] = S;
        tb_combine(q_m, q_s, tid, M, S);
        ta.dpart_m[o] = M, ta.dpart_s[o] = S;
    }
    // ---- the slice's token top-K per row: 8 threads per row, 16 consecutive columns each; K rounds of a best-untaken reduction
    const int n = tid >> 3, q = tid & 7;
    float val[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) val[i] = lg[n * LW + 16 * q + i];
    const int sym0 = slice * 32 * kGrWaves + 16 * q;
    const size_t lo = ((size_t)slice * ba.R + r0 + n) * K;
    unsigned taken = 0;
    for (int k = 0; k < K; ++k) {  // (uniform trip count: every lane takes part in the shuffles)
        float bl = -INFINITY;
        int bj = -1;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (!((taken >> i) & 1) && val[i] > bl) bl = val[i], bj = i;  // ascending symbols: the lowest wins a tie
        int bv = bj >= 0 ? sym0 + bj : INT_MAX;
        const int mine = bv;
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
            const float ol = __shfl_xor(bl, off, 8);
            const int ov = __shfl_xor(bv, off, 8);
            if (bm_better(ol, ov, bl, bv)) bl = ol, bv = ov;
        }
        if (bv != INT_MAX && bv == mine) taken |= 1u << bj;
        if (q == 0 && s_live[n]) {
            ba.pl[lo + k] = bv != INT_MAX ? bl : -INFINITY;
            ba.pv[lo + k] = bv != INT_MAX ? bv : -1;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// select: one workgroup (256 threads) per utterance
// ---------------------------------------------------------------------------------------------
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

template <bool TIMED>
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
                int ef = t, ed = d;
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

__global__ __launch_bounds__(256) void tdt_beam_select_kernel(const TdtBeamArgs ta) { tdt_beam_select_body<false>(ta); }
__global__ __launch_bounds__(256) void tdt_beam_select_timed_kernel(const TdtBeamArgs ta) { tdt_beam_select_body<true>(ta); }

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
