// beam_common.h -- what the translation units of the beam search share (beam_kernels.hip: the search; beam_bias_kernels.hip: its
// biased steps): the beam slot and the kernels' argument block, the workspace layout and its binding, and the two helpers the
// kernel bodies (beam_step_body.h, beam_select_body.h) use.  The including translation unit defines rnnt::kBeamMax and
// rnnt::kHashMul first: beam_kernels.hip is where they are set, beam_bias_kernels.hip repeats them (tests/test_context_bias.py
// holds the two against each other).
#pragma once
#include "rnnt_decode.h"

#include <limits.h>
#include <math.h>

namespace rnnt {

struct BeamSlot {
    double score;             // -inf: empty slot
    unsigned long long hash;  // rolling hash of the token sequence
    int len;                  // tokens
    int pad;
};

struct BeamArgs {
    GreedyArgs g;  // the joint's tables and image; g.st: per-utterance frame counter (t) and frames (Tb)
    BeamSlot *slot;  // [B K]
    int *nslot;      // [B] occupied slots (the first nslot[b] of the beam)
    float *pl;       // [NS][B K][K] slice top-K logits
    int *pv;         // [NS][B K][K] their symbols (-1: none)
    float *bl;       // [B K] the blank's logit (what a hypothesis with a full token row offers)
    int *tok;        // [2][B][K][N] token rows
    int2 *tt;        // timed: [2][B][K][N] {emission frame, f32 bits of the log-probability} of every token
    int *hyp_frames, *tstable;  // timed results: [B][K][N] (-1 padded), [B] (NULL: not written)
    float *hyp_logp;            // timed results: [B][K][N] (0 padded)
    int *parents, *emitted;
    float *topl, *lse;  // diagnostics (NULL: not written)
    int *tops;
    int *hyps, *hyp_lengths, *stable;
    float *scores;
    int K, R;
    int N;  // token row stride = tokens a hypothesis may hold (offline: maxT)
};

__device__ __forceinline__ bool bm_better(float l, int v, float bl, int bv) { return l > bl || (l == bl && v < bv); }

__device__ __forceinline__ int bm_token(const int *row, int len, int v, int p) {
    return p < len ? row[p] : v;  // token p of y_i + (v,): row = y_i's token row, len = |y_i|
}

// ---------------------------------------------------------------------------------------------
// the workspace
// ---------------------------------------------------------------------------------------------
size_t joint_w2_image_bytes(int J, int V);

struct BeamLayout {
    size_t st, slot, nslot, pm, ps, pl, pv, bl, tok, rowflag, expE, encraw, img, btab, tflag, tt, total;
    int NC, NS, DT;
};

// N: the token row stride (offline: T).  timed: the {frame, log-probability} rows follow the untimed layout, which stays as it
// is; the token and pair rows together are 6 B K N words, and that count must stay below 2^31
static bool make_beam_layout(int T, int B, int K, int N, int J, int V, int joint_dtype, bool timed, BeamLayout &L) {
    L.DT = greedy_dt(joint_dtype, J, V);
    if (L.DT < 0 || T <= 0 || B <= 0 || K < 1 || K > kBeamMax || N < 1) return false;
    if ((unsigned long long)B * T * J >= (1ull << 31) || (timed ? 6ull : 2ull) * B * K * N >= (1ull << 31)) return false;
    L.NC = (V + 31) / 32;
    L.NS = (L.NC + kGrWaves - 1) / kGrWaves;
    const size_t R = (size_t)B * K;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    L.st = take((size_t)B * sizeof(GreedyState));
    L.slot = take(R * sizeof(BeamSlot));
    L.nslot = take((size_t)B * sizeof(int));
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
    L.tt = timed ? take(2 * R * (size_t)N * sizeof(int2)) : off;
    L.total = off;
    return true;
}

static bool beam_bind(BeamArgs &a, int T, int B, int K, int N, int J, int V, int joint_dtype, bool timed, void *workspace,
                      BeamLayout &L) {
    if (!make_beam_layout(T, B, K, N, J, V, joint_dtype, timed, L)) return false;
    char *ws = (char *)workspace;
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
    a.tt = timed ? (int2 *)(ws + L.tt) : nullptr;
    a.K = K, a.R = B * K, a.N = N;
    return true;
}

}  // namespace rnnt
