// beam_step_body.h -- the step kernel of beam_kernels.hip, included there once per instantiation: BEAM_STEP_KERNEL is the
// kernel's name and BEAM_STEP_BIAS 0 / 1 whether it ranks on logit + beta(q, v) of the context graph bg and lists the raw logits
// (beam_step_kernel<DT> and beam_step_bias_kernel<DT>).  One source, two kernel templates with names of their own, so the
// unbiased one comes out of the compiler as it did before the biased one existed.  No include guard on purpose.
// BEAM_STEP_BIAS 2 (beam_step_lm_kernel<DT>, beam_lm_kernels.hip): bg is the n-gram LM of include/rnnt_lm.h (LmArgs) and beta its
// back-off transition; everything else is the biased kernel's.  The preprocessed text at 0 and at 1 is what it was.
// BEAM_STEP_BIAS 3 (multibeam_step_kernel<DT>, multibeam_kernels.hip: the search of include/rnnt_beam_multi.h): the unbiased kernel
// on 2 K rows per utterance, of which the first nslot[b] <= K (the open hypotheses) are live, with the blank kept out of the slice's
// top-K (its logit still goes to bl).  The preprocessed text at 0, 1 and 2 is what it was.
template <int DT>
#if BEAM_STEP_BIAS == 2
__global__ __launch_bounds__(kGrWaves * 64) void BEAM_STEP_KERNEL(const BeamArgs ba, const LmArgs bg) {
#elif BEAM_STEP_BIAS == 1
__global__ __launch_bounds__(kGrWaves * 64) void BEAM_STEP_KERNEL(const BeamArgs ba, const BiasArgs bg) {
#else
__global__ __launch_bounds__(kGrWaves * 64) void BEAM_STEP_KERNEL(const BeamArgs ba) {
#endif
    const GreedyArgs &a = ba.g;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_t[32], s_live[32], s_slow[32];
    __shared__ float r_m[kGrWaves * 64], r_s[kGrWaves * 64];
    __shared__ float stage[DT == 2 ? 32 * 33 : 1];
    __shared__ float lg[32 * (32 * kGrWaves + 1)];
#if BEAM_STEP_BIAS == 1 || BEAM_STEP_BIAS == 2
    __shared__ float bt[32 * (32 * kGrWaves + 1)];  // beta of the tile's symbols
#endif
    constexpr int LW = 32 * kGrWaves + 1;
    const int J = a.J, K = ba.K;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, n31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slice = blockIdx.x, r0 = blockIdx.y * 32;

    bool live = false;
    if (tid < 32) {
#if BEAM_STEP_BIAS == 3
        const int r = r0 + tid, b = r / (2 * K);
#else
        const int r = r0 + tid, b = r / K;
#endif
        int t = 0, slow = 0;
        if (r < ba.R) {
            const GreedyState s = a.st[b];
#if BEAM_STEP_BIAS == 3
            live = s.t < s.Tb && r - b * 2 * K < ba.nslot[b];
#else
            live = s.t < s.Tb && r - b * K < ba.nslot[b];
#endif
            t = min(max(s.t, 0), a.T - 1);
            if (live) slow = a.rowflag[(size_t)b * a.T + t];
        }
        s_live[tid] = live ? 1 : 0, s_t[tid] = t, s_slow[tid] = slow;
    }
    if (!__syncthreads_or(live)) return;  // a tile without live hypotheses reads and writes nothing
    dec_pred_route(a, J, r0, s_live, s_slow, tid);
    __syncthreads();
    gf16 *hA = (gf16 *)smem, *hL = hA + (size_t)J * 32;
    const bool hform = DT == 0 && a.tflag[1] != 0.f;
#if BEAM_STEP_BIAS == 3
    dec_build_h<DT>(a, J, r0, s_live, s_slow, [&](int n) { return (size_t)((r0 + n) / (2 * K)) * a.T + s_t[n]; }, hform, hA, hL, tid);
#else
    dec_build_h<DT>(a, J, r0, s_live, s_slow, [&](int n) { return (size_t)((r0 + n) / K) * a.T + s_t[n]; }, hform, hA, hL, tid);
#endif
    __syncthreads();

    // ---- this wave's chunk of 32 symbols: greedy's (max, sum) per lane, and the logits into lg (NaN: takes no part)
    const int vc = slice * kGrWaves + wave;
    float bm = -INFINITY, bs = 0.f;
    if (vc < a.NC) {
        const gf32x16 acc = dec_chunk_acc<DT>(a, vc, hA, hL, stage, lane);
        float m2inv, w2inv;
        dec_logit_scales<DT>(a, hform, m2inv, w2inv);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int vv = gr_cdrow(r, half), v = 32 * vc + vv;
            const float l = dec_logit<DT>(a, acc[r], vc, vv, v, m2inv, w2inv);
            if (v < a.V) {  // padding columns take no part
                if (l > bm) {
                    bs = fmaf(bs, __builtin_amdgcn_exp2f((bm - l) * kLog2e), 1.0f);
                    bm = l;
                } else {
                    bs += __builtin_amdgcn_exp2f((l - bm) * kLog2e);
                }
            }
            lg[n31 * LW + 32 * wave + vv] = v < a.V ? l : __builtin_nanf("");
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) lg[n31 * LW + 32 * wave + gr_cdrow(r, half)] = __builtin_nanf("");
    }
    r_m[tid] = bm, r_s[tid] = bs;
    __syncthreads();
    if (tid < 32 && s_live[tid] && slice == a.blank / (32 * kGrWaves)) ba.bl[r0 + tid] = lg[tid * LW + a.blank % (32 * kGrWaves)];
    if (tid < 32 && s_live[tid]) {  // the 2 kGrWaves partials of row tid, in greedy_step_kernel's order
        float M = -INFINITY;
        for (int q = 0; q < 2 * kGrWaves; ++q) {
            const int src = (q >> 1) * 64 + tid + 32 * (q & 1);
            if (r_m[src] > M) M = r_m[src];
        }
        float S = 0.f;
        for (int q = 0; q < 2 * kGrWaves; ++q) {
            const int src = (q >> 1) * 64 + tid + 32 * (q & 1);
            if (r_s[src] > 0.f) S += r_s[src] * __builtin_amdgcn_exp2f((r_m[src] - M) * kLog2e);
        }
        const size_t o = (size_t)slice * ba.R + r0 + tid;
        a.part_m[o] = M, a.part_s[o] = S;
    }
    // ---- the slice's top-K per row: 8 threads per row, 16 consecutive symbols each; K rounds of a best-untaken reduction
    const int n = tid >> 3, q = tid & 7;
#if BEAM_STEP_BIAS == 1
    {  // beta of row n's 128 symbols, by the row's 8 threads.  Row n of bt is written and read by those 8 threads ALONE, and they
       // sit in one wave (n = tid >> 3), whose LDS operations complete in the order they were issued: the three passes below
       // overwrite each other in program order without a workgroup barrier.  The s_waitcnt asm statements are compiler barriers
       // (they keep the passes' stores and the loads after them in this order), not what makes the hardware ordering hold.  A
       // change of the row-to-thread mapping that spreads a row over two waves needs __syncthreads() here instead.
        const int v0 = slice * 32 * kGrWaves;
        if (s_live[n]) {
            const int st = bg_state(bg, ba.slot[r0 + n].pad);
            const float fb = bg_fail(bg, st);
#pragma unroll
            for (int i = 0; i < 16; ++i) bt[n * LW + 16 * q + i] = v0 + 16 * q + i == a.blank ? 0.f : fb;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            int lo, hi;
            bg_arcs(bg, 0, lo, hi);  // the root's arcs of the slice: (0, v) listed -> fail_bias[q] + arc_bias
            const int rl = bg_lower(bg, lo, hi, v0), rh = bg_lower(bg, rl, hi, v0 + 32 * kGrWaves);
            for (int e = rl + q; e < rh; e += 8) {
                const int c = bg.tok[e] - v0;
                if ((unsigned)c < 32u * kGrWaves && c + v0 != a.blank) bt[n * LW + c] = st == 0 ? bg.ab[e] : fb + bg.ab[e];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (st != 0) {  // the state's own arcs win
                bg_arcs(bg, st, lo, hi);
                const int sl = bg_lower(bg, lo, hi, v0), sh = bg_lower(bg, sl, hi, v0 + 32 * kGrWaves);
                for (int e = sl + q; e < sh; e += 8) {
                    const int c = bg.tok[e] - v0;
                    if ((unsigned)c < 32u * kGrWaves && c + v0 != a.blank) bt[n * LW + c] = bg.ab[e];
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }
#endif
#if BEAM_STEP_BIAS == 2
    {  // beta of row n's 128 symbols under the LM, by the row's 8 threads: the back-off chain c_0 = q ... c_d = E of the row's
       // state is walked once (lm_backoff: the hop the select kernel takes too, so both form the same f32 sums), then the row is
       // filled with the unknown-token score and the arcs of c_d, c_(d-1), ... c_0 that fall into the slice are scattered over it,
       // the nearer level overwriting the farther.  As in the biased kernel above: row n of bt is written and read by those 8
       // threads ALONE, and they sit in one wave (n = tid >> 3), whose LDS operations complete in the order they were issued, so
       // the fill and EVERY pass of the level loop overwrite each other in program order without a workgroup barrier.  The
       // s_waitcnt asm statements are compiler barriers (they keep each pass's stores, the next pass's stores and the loads
       // after the loop in this order), not what makes the hardware ordering hold.  A change of the row-to-thread mapping that
       // spreads a row over two waves needs __syncthreads() after the fill and after every level instead.
        const int v0 = slice * 32 * kGrWaves;
        if (s_live[n]) {
            int c[RNNT_LM_MAX_HOPS + 1];
            float ac[RNNT_LM_MAX_HOPS + 1];
            int cur = bg_state(bg, ba.slot[r0 + n].pad), hop = 0;
            float acc = 0.f;
            c[0] = cur, ac[0] = 0.f;
#pragma unroll
            for (int h = 1; h <= RNNT_LM_MAX_HOPS; ++h) {  // (static indices: the chain stays in registers)
                if (cur != bg.E) lm_backoff(bg, cur, acc, hop);
                c[h] = cur, ac[h] = acc;
            }
            const int d = hop;  // c[d] == E
            const float unk = d == 0 ? bg.unk : acc + bg.unk;
#pragma unroll
            for (int i = 0; i < 16; ++i) bt[n * LW + 16 * q + i] = v0 + 16 * q + i == a.blank ? 0.f : unk;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int j = RNNT_LM_MAX_HOPS; j >= 0; --j) {
                if (j <= d) {  // (uniform over the row's 8 threads)
                    int lo, hi;
                    bg_arcs(bg, c[j], lo, hi);
                    const int sl = bg_lower(bg, lo, hi, v0), sh = bg_lower(bg, sl, hi, v0 + 32 * kGrWaves);
                    for (int e = sl + q; e < sh; e += 8) {
                        const int col = bg.tok[e] - v0;
                        if ((unsigned)col < 32u * kGrWaves && col + v0 != a.blank) bt[n * LW + col] = j == 0 ? bg.sc[e] : ac[j] + bg.sc[e];
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        }
    }
#endif
    float val[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) val[i] = lg[n * LW + 16 * q + i];
#if BEAM_STEP_BIAS == 1 || BEAM_STEP_BIAS == 2
    if (s_live[n]) {  // the key
#pragma unroll
        for (int i = 0; i < 16; ++i) val[i] += bt[n * LW + 16 * q + i];
    }
#endif
    const int sym0 = slice * 32 * kGrWaves + 16 * q;
#if BEAM_STEP_BIAS == 3
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (sym0 + i == a.blank) val[i] = __builtin_nanf("");  // the blank closes a hypothesis: it is no expansion
#endif
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
#if BEAM_STEP_BIAS == 1 || BEAM_STEP_BIAS == 2
            ba.pl[lo + k] = bv != INT_MAX ? lg[n * LW + bv - slice * 32 * kGrWaves] : -INFINITY;  // (raw, in key order)
#else
            ba.pl[lo + k] = bv != INT_MAX ? bl : -INFINITY;
#endif
            ba.pv[lo + k] = bv != INT_MAX ? bv : -1;
        }
    }
}
