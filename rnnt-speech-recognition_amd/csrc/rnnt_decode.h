// rnnt_decode.h -- the per-hypothesis joint of the decoders (greedy_kernels.hip, beam_kernels.hip), shared so that both see
// bitwise the logits of compute_rnnt_joint_logits for one hypothesis alone (see greedy_kernels.hip for the arithmetic).
//
// A step workgroup owns 32 hypothesis rows (the 32 columns of v_mfma_f32_32x32x16_f16) and a slice of kGrWaves vocabulary
// chunks of 32 symbols, one per wave.  The pieces, in the order a step kernel calls them:
//   dec_pred_route   the pred-side half of the per-hypothesis tanh route switch (8 threads per row scan its pred_proj row)
//   dec_build_h      h (DT 1) or r / h split into hi + lo (DT 0 / 2) of the 32 rows, in B-fragment order, into LDS
//   dec_chunk_acc    the MFMA chains of this wave's chunk (DT 2: transposed through LDS), lane n31 = row, symbols gr_cdrow
//   dec_logit        the epilogue arithmetic: accumulator -> f32 logit
#pragma once

#include "rnnt_common.h"
#include "rnnt_joint_math.h"

namespace rnnt {

typedef _Float16 gf16;
typedef _Float16 gh8 __attribute__((ext_vector_type(8)));
typedef float gf32x16 __attribute__((ext_vector_type(16)));

constexpr int kGrWaves = 4;  // waves per step workgroup: wave w of slice s takes vocabulary chunk kGrWaves s + w

// per-hypothesis decoder state (workspace).  The beam decoder keeps one per utterance and uses t / Tb (its frame counter).
struct GreedyState {
    int t;       // current frame
    int n;       // symbols emitted
    int nf;      // symbols emitted at the current frame
    int done;    // 1: t >= Tb or n >= maxsym
    int Tb;      // frames of the utterance (clamped to [0, maxT])
    int maxsym;  // symbol budget (clamped to >= 0; INT_MAX: none)
    int cap;     // symbols per frame at most (<= 0: no cap)
    int fin;     // stream decoder: 1 once the stream has finished (its final chunk fed, or its budget spent) until a reset
    double score;  // sum of the log-softmax of every decision taken
};

struct GreedyArgs {
    const float *enc_proj, *W2, *b2;
    const int *frame_lengths, *max_symbols;
    const float *pred_proj;
    int *hyps, *hyp_lengths, *emitted, *all_done;
    float *scores, *stats;
    GreedyState *st;
    float *part_m, *part_s;
    int *part_i;
    int *rowflag;      // [B][T] 1: some |enc_proj| of the row beyond kExpTabLimit (or NaN)
    float *expE;       // [B][T][J] e^{2 enc_proj}
    float *encraw;     // [B][T][J] enc_proj (the direct-tanh route)
    gf16 *img;         // W2 operand image: DT 1 [NC][J/16][2][32][8] binary16; DT 0 / 2 joint_prep_kernel's W2s
    float *btab;       // DT 1: b2 log2 e [NC 32]; DT 2: b2 [32]
    const float *tflag;  // DT 0 / 2: joint_prep_kernel's flag words (+ 64: b2s)
    int B, T, J, V, NC, NS, blank, max_per_frame, max_hyp_len;
    // the timed step (greedy_update_timed_kernel): per token the frame that emitted it and the log-softmax of that decision,
    // at the token's position in hyps
    int *hyp_frames;        // [B][max_hyp_len]
    float *hyp_logp;        // [B][max_hyp_len]
    const int *frame_base;  // [B] frames of the stream's earlier chunks (NULL: 0)
};

__device__ __forceinline__ constexpr int gr_cdrow(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// the pred-side half of the route switch: 8 threads per row scan pred_proj row row0 + n
__device__ __forceinline__ void dec_pred_route(const GreedyArgs &a, const int J, const int row0, const int *s_live, int *s_slow,
                                               const int tid) {
    const int n = tid >> 3, q = tid & 7;
    bool big = false;
    if (s_live[n])
        for (int j = q; j < J; j += 8) big |= exp_tab_out_of_range(a.pred_proj[(size_t)(row0 + n) * J + j]);
    if (big) s_slow[n] = 1;
}

// h (DT 1) or r / h split into hi + lo (DT 0 / 2), in B-fragment order: lane n + 32 half of k-step ks holds units
// 16 ks + 8 half + 0..7 of row n.  erow(n): the row of the enc tables ([B][T]) row n reads.  Rows not live get h = 0.
template <int DT, class ERow>
__device__ __forceinline__ void dec_build_h(const GreedyArgs &a, const int J, const int row0, const int *s_live, const int *s_slow,
                                            ERow erow, const bool hform, gf16 *hA, gf16 *hL, const int tid) {
    for (int i = tid; i < 32 * J; i += kGrWaves * 64) {
        const int n = i / J, j = i - n * J;
        float x = 0.f;
        if (s_live[n]) {
            const size_t er = erow(n) * J + j;
            const float pv = a.pred_proj[(size_t)(row0 + n) * J + j];
            if (!s_slow[n]) {
                const float ea = a.expE[er], ec = exp_tab(pv);
                x = DT == 0 ? r_from_exp(ea, ec) : tanh_from_exp(ea, ec);
            } else {
                const float ev = a.encraw[er];
                x = DT == 0 ? fast_r(ev + pv) : fast_tanh(ev + pv);
            }
            if (hform) x = fmaf(x, -2.0f, 1.0f);
        }
        const int off = (((j >> 4) * 64 + n + 32 * ((j >> 3) & 1)) << 3) + (j & 7);
        const gf16 hi = (gf16)x;
        hA[off] = hi;
        if (DT != 1) hL[off] = (gf16)(x - (float)hi);  // exact residual in f32, then rounded: split_pair's hi / lo
    }
}

// the product of vocabulary chunk vc against the 32 rows; afterwards lane n31 holds row n31, symbols 32 vc + gr_cdrow(r, half).
// stage: DT 2's transpose buffer, 32 x 33 floats (DT 2 has one chunk: only wave 0 gets here)
template <int DT>
__device__ __forceinline__ gf32x16 dec_chunk_acc(const GreedyArgs &a, const int vc, const gf16 *hA, const gf16 *hL, float *stage,
                                                 const int lane) {
    const int J = a.J, KS = J >> 4, half = lane >> 5, n31 = lane & 31;
    gf32x16 acc;
    const gh8 *hb = (const gh8 *)hA + lane, *hl = (const gh8 *)hL + lane;
    if (DT == 1) {
        const gh8 *w = (const gh8 *)a.img + (size_t)vc * KS * 64 + lane;
        gf32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = 0.f, acc1[r] = 0.f;
        for (int ks = 0; ks < KS; ks += 2) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[ks * 64], hb[ks * 64], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[(ks + 1) * 64], hb[(ks + 1) * 64], acc1, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = acc0[r] + acc1[r];
    } else {
        const gh8 *w = (const gh8 *)a.img + (size_t)vc * J * 8 + lane;  // tile vc: [J/16][hi, lo][64 lanes] fragments
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int ks = 0; ks < KS; ++ks) {
            const gh8 wh = w[(2 * ks) * 64], wl = w[(2 * ks + 1) * 64], bh = hb[ks * 64], bl = hl[ks * 64];
            if (DT == 0) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, bh, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, bl, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, bh, acc, 0, 0, 0);
            } else {  // h as the A operand: D[hypothesis][symbol]
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, wh, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl, wh, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, wl, acc, 0, 0, 0);
            }
        }
    }
    if (DT == 2) {  // transpose through LDS: afterwards lane n31 holds hypothesis n31, symbols gr_cdrow(r, half), as for DT 0 / 1
#pragma unroll
        for (int r = 0; r < 16; ++r) stage[gr_cdrow(r, half) * 33 + n31] = acc[r];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (one wave: its LDS operations complete in order)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = stage[n31 * 33 + gr_cdrow(r, half)];
    }
    return acc;
}

// the epilogue's scale of the accumulator (DT 0: m2inv, DT 2: w2inv)
template <int DT>
__device__ __forceinline__ void dec_logit_scales(const GreedyArgs &a, const bool hform, float &m2inv, float &w2inv) {
    m2inv = 0.f;
    if (DT == 0) m2inv = hform ? a.tflag[2] : -2.0f * a.tflag[2];
    w2inv = DT == 2 ? a.tflag[2] : 0.f;
}

// logit of symbol v = 32 vc + vv from its accumulator
template <int DT>
__device__ __forceinline__ float dec_logit(const GreedyArgs &a, const float acc, const int vc, const int vv, const int v,
                                           const float m2inv, const float w2inv) {
    if (DT == 1) return fmaf(acc, kLog2e, a.btab[v]) * kLn2;
    if (DT == 0) return fmaf(acc, m2inv, a.tflag[64 + 64 * vc + vv]) + a.tflag[64 + 64 * vc + 32 + vv];
    return fmaf(acc, w2inv, a.btab[v]);
}

// the stream decoders' feed (greedy_kernels.hip greedy_stream_*, beam_kernels.hip beam_stream_*): a chunk of encoder frames per slot
struct GreedyStreamArgs {
    const float *enc;          // [S, Te, H]
    const float *W1, *b1;      // workspace copies: [H][J], [J]
    const int *chunk_frames, *reset, *final_, *max_symbols;
    int *hyp_lengths, *all_done;
    float *scores;
    GreedyState *st;
    int *rowflag;
    float *expE, *encraw;
    int S, Te, T, H, J, max_per_frame;
    int *frame_base;  // the timed feed (greedy_stream_feed_timed_kernel): [S] frames of the chunks fed before this one
};

__device__ __forceinline__ int gs_frames(const GreedyStreamArgs &a, const int s) { return min(max(a.chunk_frames[s], 0), a.Te); }

// host side: the prepare path (greedy_kernels.hip) both decoders run in their begin.  DT: 0 / 1 / 2 of the step kernels.
// greedy_dt: DT for (joint_dtype, J, V), or -1 when the shape is not taken.
int greedy_dt(int joint_dtype, int J, int V);
hipError_t launch_greedy_prepare(const GreedyArgs &a, int DT, const float *W2, const float *b2, hipStream_t s);
// the pieces of the greedy stream that the beam stream runs unchanged (greedy_kernels.hip): the W2 image alone; W1 [H][J] / b1 [J]
// copied to w1 / bb1 with st[0 .. S) set finished (b2 / btab: DT 2's bias table, else NULL); greedy_stream_proj_kernel over a.enc
hipError_t launch_greedy_w2(const GreedyArgs &a, int DT, const float *W2, const float *b2, hipStream_t s);
hipError_t launch_greedy_stream_pack(const float *W1, const float *b1, float *w1, float *bb1, int H, int J, GreedyState *st, int S,
                                     const float *b2, float *btab, int V, hipStream_t s);
hipError_t launch_greedy_stream_proj(const GreedyStreamArgs &a, hipStream_t s);

}  // namespace rnnt
