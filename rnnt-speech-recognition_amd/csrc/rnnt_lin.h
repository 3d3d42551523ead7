// rnnt_lin.h -- the LINEAR-domain lattice of the small-vocabulary loss path (round 4): shared definitions and the per-cell
// device code of the two cell passes.  Replaces the same stages of warp-transducer's GPU path as rnnt_kernels.hip does
// (SURVEY.md 2.1, 8a-6 ... a-9; call site utils/loss.py:34-35), with the transcendentals taken off the sweeps' serial chain:
//
//   lsm pass    edge PROBABILITIES {p(blank), p(label)} per cell (zeros where an edge leaves the lattice), no lse store
//   sweeps      alpha^ / beta^ as float32 mantissas x 2^frame, one integer frame per sweep lane (K lattice columns) and block
//               of kLinR diagonals: the step is multiply / add only, the renormalisation is exact (powers of two)
//   grad pass   softmax numerators recomputed from the logits it reads anyway; occupancies formed from mantissas + frames
//
// Fixed frames can lose mass that falls more than 126 bits below its lane's frame.  Whether that mattered is decided per cell
// by the gradient pass (lin_certificate below: what a flush can have cost, times the other side's mass, over the likelihood)
// and per utterance by the sweeps (non-finite / zero likelihood, alpha-side vs beta-side likelihood).  An utterance that fails
// is redone in the log domain by lin_redo_kernel (rnnt_lin_kernels.hip) -- log2 values, recurrence in float64 (rnnt_sweep.h alpha_sweep_pr), any range -- so the
// results never depend on the shortcut.  tests/tools/emulate_linear.py restates all of it in NumPy.
#pragma once
#include "rnnt_sweep.h"

namespace rnnt {

// Diagonals per frame block: a lane renormalises (and the frame tables get a row) every 2^shift diagonals.  The renormalisation
// is ~22 instructions of the sweeping wave (4 us of the sweep at B32 T600 U150 with blocks of four), so blocks are EIGHT diagonals
// long where the mass decays slowly and FOUR where it decays fast -- chosen per utterance by the sweeps from a statistic the lsm
// pass leaves behind: the mean of -log2 max(p_blank, p_label) over the utterance's cells (bits of mass lost per diagonal along the
// better edge).  N(0,1) logits: 4.7 bits at 28 symbols, 5.8 at 60 (certificate margin -84 / -72 bits with blocks of eight);
// trained-like posteriors 0 ... 3; 3 x N(0,1): 7.3 (margin -43 with blocks of eight, -69 with four); 4 x N(0,1): 9.1 (-45 with four).
// K = 1, 12, 16: always four (K = 1: the frame look-back would be 8 lanes deep; 12, 16: their LDS chunks are four diagonals long).
__host__ __device__ constexpr int lin_shift_max(int K) { return (K == 1 || K >= 12) ? 2 : 3; }
constexpr float kLinDecayBits = 6.2f;  // mean bits per diagonal beyond which an utterance gets blocks of four
constexpr int kLinDrag = 118;            // a lane's frame is at most this far below the lanes mass can reach it from within a block
constexpr int kFrameNone = -(1 << 28);   // frame of a lane without mass and without a neighbour to copy from
constexpr int kCertBits = -40;           // per-cell bound (bits) on flush loss x other side / likelihood
constexpr float kTinyEdge = 7.8886091e-31f;  // 2^-100: an edge the lattice owns below this goes to the log-domain path (NaN in W)

// per-utterance words in LossParams::flags
enum { kFlagA = 0, kFlagB = 1, kFlagG = 2, kFlagState = 3 };  // state: 0 linear lattice, 2 log-domain lattice ready (after a redo)

__device__ __forceinline__ void st_i32_wt(int *q, int v) { __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float frexp_m(float x) { return __builtin_amdgcn_frexp_mantf(x); }  // in [0.5, 1); 0 -> 0
__device__ __forceinline__ int frexp_e(float x) { return __builtin_amdgcn_frexp_expf(x); }      // 0 for x == 0
__device__ __forceinline__ float ldexp_f(float x, int e) { return __builtin_ldexpf(x, e); }     // v_ldexp_f32

// True when the utterance's lattice is not (or no longer) in the linear format: the fast gradient pass leaves it alone.
// The four flag words of an utterance are one 16-byte (scalar) load: `a || b` on single words was two dependent trips.
__device__ __forceinline__ bool lin_skip_words(const int4 fl) { return (fl.x | fl.y) != 0 || fl.w == 2; }  // kFlagA, kFlagB, kFlagState
__device__ __forceinline__ int4 lin_flag_words(const LossParams &p, const int b) { return *(const int4 *)(p.flags + 4 * b); }
__device__ __forceinline__ bool lin_skip(const LossParams &p, const int b) { return lin_skip_words(lin_flag_words(p, b)); }

// What the gradient pass reads per UTTERANCE (workgroup-uniform: scalar loads), fetched in one batch with the flag words and the
// lengths at the top of the patch kernel, in front of the decision whether the utterance is skipped.
struct LinUtt {
    int sh;       // log2 of the diagonals per frame block the sweeps chose
    float mL;     // the likelihood: mantissa ...
    int EL;       // ... and frame
    float scale;  // cost_scale[b], 1 without one
};

// ---- where the gradient set-up of cell (b, n = t + u, u) reads: index arithmetic alone, checked on the host over whole lattices
// (tests/test_cell_prologue_host.py).  The set-up fetches all of it unconditionally, so every index is clamped into its array;
// a clamp is only ever active for an edge the cell does not have, whose value a select then discards. ----
struct LinIdx {
    size_t sk;                  // A, Bt: the cell
    size_t down;                // Bt: (t + 1, u), row n + 1 (row Nr does not exist: clamped to the cell's own row)
    size_t diag;                // Bt: (t, u + 1), row n + 1, column u + 1 (column Up does not exist)
    size_t e00, e10, e11;       // frame tables [B][NCl][64]: (kc, l0), (kc1, l0), (kc1, l1)
    size_t lab;                 // labels [B][U - 1]: (b, u), u clamped to U - 2; not to be used when U == 1 (no label array)
};
__host__ __device__ __forceinline__ LinIdx lin_grad_indices(const int b, const int n, const int u, const int sh, const int l0, const int l1,
                                                            const int Nr, const int Up, const int NCl, const int U) {
    LinIdx x;
    const int n1 = n + 1 < Nr ? n + 1 : Nr - 1, u1 = u + 1 < Up ? u + 1 : Up - 1;
    x.sk = ((size_t)b * Nr + n) * Up + u;
    x.down = ((size_t)b * Nr + n1) * Up + u;
    x.diag = ((size_t)b * Nr + n1) * Up + u1;
    const int kc = n >> sh, kc1 = (n + 1) >> sh;
    const int kcc = kc < NCl ? kc : NCl - 1, kc1c = kc1 < NCl ? kc1 : NCl - 1;
    const int l1c = l1 < 64 ? l1 : 63;
    const size_t tb = (size_t)b * NCl * 64;
    x.e00 = tb + (size_t)kcc * 64 + l0;
    x.e10 = tb + (size_t)kc1c * 64 + l0;
    x.e11 = tb + (size_t)kc1c * 64 + l1c;
    const int ul = u < U - 2 ? u : U - 2;
    x.lab = (size_t)b * (U - 1) + (ul > 0 ? ul : 0);
    return x;
}

// ---- lsm: one valid cell, its V logits in x[] (registers) and at xs (its slot of the patch image in LDS) ----
// Returns -log2 max(p_blank, p_label) of the cell (the decay statistic; 200 where an edge had to be refused).
// `lab`: the cell's clamped label, fetched by the caller BEFORE it staged the logits (it depends on (b, u) alone; loaded here,
// between the staging barrier and the edge-store barrier, it cost every workgroup a global-memory round trip with its LDS held);
// looked at only where u < U_b - 1.
template <int VP>
__device__ __forceinline__ float lin_cell_lsm(const LossParams &p, const Cell &cl, const float (&x)[VP], const float *xs, const int lab) {
    float m = x[0];
#pragma unroll
    for (int i = 1; i < VP; ++i) m = fmaxf(m, x[i]);
    float s = 0.f;
    const float nml = -m * kLog2e;
#pragma unroll
    for (int i = 0; i < VP; ++i) s += ex2(fmaf(x[i], kLog2e, nml));
    const float inv = __builtin_amdgcn_rcpf(s);
    // a blank from the last frame leaves the lattice unless it is THE terminal transition
    const bool blank_stays = (cl.t < cl.Tb - 1) || (cl.u == cl.Ub - 1);
    float pb = 0.f, pl = 0.f;
    if (blank_stays) {
        pb = ex2(fmaf(xs[p.blank], kLog2e, nml)) * inv;
        if (!(pb >= kTinyEdge)) pb = NAN;  // (also a NaN logit): not representable here -> the sweeps hand the utterance back
    }
    if (cl.u < cl.Ub - 1) {
        pl = ex2(fmaf(xs[lab], kLog2e, nml)) * inv;
        if (!(pl >= kTinyEdge)) pl = NAN;
    }
    // The two edge probabilities go into the first two floats of the cell's own LDS slot (nobody else reads it); the patch kernel
    // writes them to the skewed edge array diagonal by diagonal afterwards (rnnt_kernels.hip: consecutive lanes then store
    // consecutive positions of one diagonal's row -- written from here, a lane per cell, every store of a wave went to 64 rows).
    float *const xo = const_cast<float *>(xs);
    xo[0] = pb, xo[1] = pl;
    const float best = fmaxf(pb, pl);  // (v_max ignores a NaN operand)
    return (pb != pb || pl != pl) ? 200.f : -lg2(fmaxf(best, 1.0e-37f));
}

// ---- gradient set-up of one valid cell from mantissas + frames ----
struct LinGrad {
    float h0;  // cost_scale * occupancy            (x e_v / s = the softmax term)
    float hb;  // cost_scale * alpha p(..) beta(t+1,u) / L without the p: multiplies e_blank / s
    float hl;  // the same for the label edge
    float l2occ;  // log2 of the occupancy alpha beta / L (no cost_scale): the occupancy floor of the gradient pass (rnnt_kernels.hip)
    bool has_blank_corr, has_label, bad;
    int lab;
};

// Everything the cell needs from global memory is asked for in ONE batch -- the cell, both neighbours of the next diagonal, the four
// frames, the label -- unconditionally and with clamped indices (lin_grad_indices), and waited for once: fetched inside the
// `t < T_b - 1` / `has_label` branches they were three dependent round trips (to values another XCD wrote write-through) in front of
// the first logit of every patch -- and the whole life of a dead one.  What was fetched for an edge the cell does not have is
// replaced by zero BEFORE any arithmetic (the workspace may hold NaN there).
__device__ __forceinline__ LinGrad lin_grad_setup(const LossParams &p, const Cell &cl, const LinUtt &ut) {
    LinGrad g;
    const int n = cl.t + cl.u;
    const int l0 = (int)fdiv((uint32_t)cl.u, p.divOG), l1 = (int)fdiv((uint32_t)cl.u + 1u, p.divOG);
    const LinIdx ix = lin_grad_indices(cl.b, n, cl.u, ut.sh, l0, l1, p.Nr, p.Up, p.NCl, p.U);
    const float ma = p.A[ix.sk], mb = p.Bt[ix.sk];
    const float m_dn = p.Bt[ix.down], m_dg = p.Bt[ix.diag];
    const int ea = p.EA[ix.e00], eb = p.EB[ix.e00];
    const int e_dn = p.EB[ix.e10], e_dg = p.EB[ix.e11];
    // (U == 1: there is no label array and no cell has a label -- some readable word instead of a branch, which would close the batch)
    const int labw = *(p.U > 1 ? p.labels + ix.lab : (const int *)p.lshift + cl.b);
    const bool down = cl.t < cl.Tb - 1;
    g.has_label = cl.u < cl.Ub - 1;
    const float mL = ut.mL;
    const int EL = ut.EL;
    const float scale = ut.scale;
    // alpha / L as (qa, base): mantissas may sit anywhere in the f32 range (a dragged frame), so split before multiplying
    const int xa = frexp_e(ma), xb = frexp_e(mb);
    const float qa = scale * frexp_m(ma) * __builtin_amdgcn_rcpf(mL);
    const int base = ea + xa - EL;
    g.h0 = ldexp_f(qa * frexp_m(mb), base + eb + xb);
    // (a zero mantissa gives -inf: dead; a NaN or infinite likelihood / mantissa gives NaN or +inf: live)
    g.l2occ = lg2(frexp_m(ma) * frexp_m(mb) * __builtin_amdgcn_rcpf(mL)) + (float)(ea + xa + eb + xb - EL);
    {
        const float m1 = down ? m_dn : 0.f;
        const int e1 = down ? e_dn : 0;
        const float via = ldexp_f(qa * frexp_m(m1), base + e1 + frexp_e(m1));
        const bool term = cl.u == cl.Ub - 1;  // the terminal transition: beta of the virtual end node is 1
        g.has_blank_corr = down || term;
        g.hb = down ? via : (term ? ldexp_f(qa, base) : 0.f);
    }
    {
        const float m1 = g.has_label ? m_dg : 0.f;
        const int e1 = g.has_label ? e_dg : 0;
        const float via = ldexp_f(qa * frexp_m(m1), base + e1 + frexp_e(m1));
        g.lab = g.has_label ? clamp_label(labw, p.V) : 0;
        g.hl = g.has_label ? via : 0.f;
    }
    // Certificate.  A product or sum below 2^-126 of its frame is flushed (or loses bits as a denormal): alpha^ of this cell is
    // short of alpha by at most ~2^(ea-126), which can reach the likelihood through at most beta(cell); the same for beta^; and
    // where both sides are zero, through 2^(ea-126) 2^(eb-126).  All three must be negligible against the likelihood.
    int worst = ea + eb - 252 - EL;
    if (mb != 0.f) worst = max(worst, ea - 126 + eb + xb - EL);
    if (ma != 0.f) worst = max(worst, eb - 126 + ea + xa - EL);
    g.bad = worst > kCertBits || !(ma <= FLT_MAX) || !(mb <= FLT_MAX) || !(ma >= 0.f) || !(mb >= 0.f);
    return g;
}

}  // namespace rnnt
