// tdt_beam_step_body.h -- the step kernel of the TDT beam searches, textually shared: tdt_beam_kernels.hip compiles it as
// tdt_beam_step_kernel (TDT_BEAM_STEP_STREAM 0), tdt_nbest_stream_kernels.hip as tdt_beam_stream_step_kernel (1), which also stores
// the blank's logit of every active row into BeamArgs::bl.  The includer defines TDT_BEAM_STEP_KERNEL and TDT_BEAM_STEP_STREAM,
// and has included tdt_beam_common.h.  What the kernel does: the head of tdt_beam_kernels.hip.
#ifndef TDT_BEAM_STEP_HELPERS
#define TDT_BEAM_STEP_HELPERS
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
#endif  // TDT_BEAM_STEP_HELPERS

template <int DT>
__global__ __launch_bounds__(kGrWaves * 64) void TDT_BEAM_STEP_KERNEL(const TdtBeamArgs ta) {
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
#if TDT_BEAM_STEP_STREAM  // the blank's logit of every active row: what a hypothesis with a full token row offers (beam_step_body.h)
    if (tid < 32 && s_live[tid] && slice == a.blank / (32 * kGrWaves)) ba.bl[r0 + tid] = lg[tid * LW + a.blank % (32 * kGrWaves)];
#endif
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
