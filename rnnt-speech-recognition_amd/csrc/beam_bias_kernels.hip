// beam_bias_kernels.hip -- contextual biasing of the beam searches (include/rnnt_bias.h): the biased step and select kernels and
// their launch.  A translation unit of its own, so that beam_kernels.hip compiles to what it compiled to before: the kernels here
// are beam_step_body.h / beam_select_body.h with the bias flag set (beam_step_bias_kernel<DT>, beam_select_bias_kernel and its
// timed twin) on the workspace beam_kernels.hip lays out (beam_common.h).
//
// A deterministic automaton over token ids (rnntBiasGraph) adds a bonus beta(q_i, v) to the key a candidate is ranked by and to
// its score; the automaton state q_i of a hypothesis lives in BeamSlot::pad (0 = the root: what every begin and reset kernel
// writes), so no workspace layout changes.  The step forms beta for the tile's [32 rows][128 symbols] in LDS (the fail bias on
// the non-blank columns, then the root's and the state's arcs that fall into the slice, found by bisection and scattered by the
// 8 threads of a row), ranks on logit + beta and lists the RAW logits in key order; the select re-derives beta and the next
// state for the listed entries by bisection.
#include "../../include/rnnt_bias.h"
#include "rnnt_decode.h"

namespace rnnt {
// (as beam_kernels.hip sets them)
constexpr int kBeamMax = 16;
constexpr unsigned long long kHashMul = 0x9E3779B97F4A7C15ull;
}  // namespace rnnt

#include "beam_common.h"

namespace rnnt {

// the context graph of the biased step (rnntBiasGraph) and where the states go; every index read from it is clamped
struct BiasArgs {
    const int *off, *tok, *nxt;
    const float *ab, *fb;
    int *states;  // [B K] (NULL: not written)
    int S, A;
};

__device__ __forceinline__ int bg_state(const BiasArgs &g, int q) { return min(max(q, 0), g.S - 1); }
__device__ __forceinline__ float bg_fail(const BiasArgs &g, int q) { return g.fb ? g.fb[q] : 0.f; }  // (NULL: a graph without arcs)

// the arcs of state s: [lo, hi) within [0, A)
__device__ __forceinline__ void bg_arcs(const BiasArgs &g, int s, int &lo, int &hi) {
    lo = hi = 0;
    if (g.A == 0) return;  // (the arc arrays may be NULL)
    lo = min(max(g.off[s], 0), g.A);
    hi = min(max(g.off[s + 1], lo), g.A);
}

// the first arc of [lo, hi) whose token is >= v (tokens ascend)
__device__ __forceinline__ int bg_lower(const BiasArgs &g, int lo, int hi, int v) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (g.tok[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int bg_find(const BiasArgs &g, int s, int v) {  // the arc (s, v), or -1
    int lo, hi;
    bg_arcs(g, s, lo, hi);
    const int a = bg_lower(g, lo, hi, v);
    return a < hi && g.tok[a] == v ? a : -1;
}

// delta(q, v) of include/rnnt_bias.h -> beta; next: the new state
__device__ __forceinline__ float bg_delta(const BiasArgs &g, int q, int v, int blank, int &next) {
    next = q;
    if (v == blank) return 0.f;
    int a = bg_find(g, q, v);
    if (a >= 0) {
        next = bg_state(g, g.nxt[a]);
        return g.ab[a];
    }
    const float fb = bg_fail(g, q);
    next = 0;
    if (q == 0) return fb;
    a = bg_find(g, 0, v);
    if (a < 0) return fb;
    next = bg_state(g, g.nxt[a]);
    return fb + g.ab[a];
}

#define BEAM_STEP_KERNEL beam_step_bias_kernel
#define BEAM_STEP_BIAS 1
#include "beam_step_body.h"
#undef BEAM_STEP_KERNEL
#undef BEAM_STEP_BIAS

#define BEAM_SELECT_KERNEL beam_select_bias_kernel
#define BEAM_SELECT_TIMED 0
#define BEAM_SELECT_BIAS 1
#include "beam_select_body.h"
#undef BEAM_SELECT_KERNEL
#undef BEAM_SELECT_TIMED
#define BEAM_SELECT_KERNEL beam_select_timed_bias_kernel
#define BEAM_SELECT_TIMED 1
#include "beam_select_body.h"
#undef BEAM_SELECT_KERNEL
#undef BEAM_SELECT_TIMED
#undef BEAM_SELECT_BIAS

template <int DT>
static hipError_t launch_beam_step_bias_dt(const BeamArgs &a, const BiasArgs &bg, size_t shm, hipStream_t s) {
    const hipError_t e = set_lds(beam_step_bias_kernel<DT>, shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(beam_step_bias_kernel<DT>, dim3(a.g.NS, (a.R + 31) / 32), dim3(kGrWaves * 64), shm, s, a, bg);
    return hipGetLastError();
}

// the biased step (include/rnnt_bias.h): graph checked by the caller, bias_states [B K] or NULL
hipError_t launch_beam_step_biased(const float *pred_proj, int *parents, int *emitted, float *topk_logits, int *topk_symbols,
                                   float *lse, int J, int V, int B, int T, int K, int N, int blank, int joint_dtype, bool timed,
                                   void *workspace, hipStream_t s, const rnntBiasGraph *graph, int *bias_states) {
    BeamArgs a = {};
    BeamLayout L;
    if (!beam_bind(a, T, B, K, N, J, V, joint_dtype, timed, workspace, L)) return hipErrorInvalidValue;
    a.g.pred_proj = pred_proj, a.g.blank = blank;
    a.parents = parents, a.emitted = emitted, a.topl = topk_logits, a.tops = topk_symbols, a.lse = lse;
    BiasArgs bg = {};
    bg.off = graph->arc_offsets, bg.tok = graph->arc_tokens, bg.nxt = graph->arc_next;
    bg.ab = graph->arc_bias, bg.fb = graph->fail_bias, bg.states = bias_states;
    bg.S = graph->num_states, bg.A = graph->num_arcs;
    hipError_t e;
    const size_t shm = (size_t)J * 32 * sizeof(gf16) * (L.DT == 1 ? 1 : 2);
    if (L.DT == 1) e = launch_beam_step_bias_dt<1>(a, bg, shm, s);
    else if (L.DT == 0) e = launch_beam_step_bias_dt<0>(a, bg, shm, s);
    else e = launch_beam_step_bias_dt<2>(a, bg, shm, s);
    if (e != hipSuccess) return e;
    if (timed) hipLaunchKernelGGL(beam_select_timed_bias_kernel, dim3(B), dim3(256), 0, s, a, bg);
    else hipLaunchKernelGGL(beam_select_bias_kernel, dim3(B), dim3(256), 0, s, a, bg);
    return hipGetLastError();
}

}  // namespace rnnt
