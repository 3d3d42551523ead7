// beam_lm_kernels.hip -- n-gram language-model shallow fusion in the beam searches (include/rnnt_lm.h): the LM step and select
// kernels and their launch.  A translation unit of its own, as beam_bias_kernels.hip is, so that beam_kernels.hip and
// beam_bias_kernels.hip compile to what they compiled to before: the kernels here are beam_step_body.h / beam_select_body.h in
// their third mode (beam_step_lm_kernel<DT>, beam_select_lm_kernel and its timed twin) on the workspace beam_kernels.hip lays
// out (beam_common.h).
//
// A back-off n-gram LM as a deterministic automaton over token ids (rnntLmGraph) adds its score beta(q_i, v) to the key a
// candidate is ranked by and to its score; the state q_i of a hypothesis lives in BeamSlot::pad (0 = the sentence-start state:
// what every begin and reset kernel writes), so no workspace layout changes.  A token the state does not list follows the
// chain of back-off states down to the state E of the empty history, a back-off score added per hop.  The step walks that chain
// once per row and forms beta for the tile's [32 rows][128 symbols] in LDS (the unknown-token score on the non-blank columns,
// then the arcs of the chain's states that fall into the slice, the farthest level first, found by bisection and scattered by
// the 8 threads of a row), ranks on logit + beta and lists the RAW logits in key order; the select re-derives beta and the next
// state for the listed entries by the same walk.  Both take their hops with lm_backoff, so the step's key and the select's are
// the same f32.
#include "../../include/rnnt_lm.h"
#include "rnnt_decode.h"

namespace rnnt {
// (as beam_kernels.hip sets them)
constexpr int kBeamMax = 16;
constexpr unsigned long long kHashMul = 0x9E3779B97F4A7C15ull;
}  // namespace rnnt

#include "beam_common.h"

namespace rnnt {

// the LM of the fused step (rnntLmGraph) and where the states go; every index read from it is clamped
struct LmArgs {
    const int *off, *tok, *nxt, *bn;
    const float *sc, *bs;
    int *states;  // [B K] (NULL: not written)
    int S, A, E;  // (E clamped by the launch)
    float unk;
};

__device__ __forceinline__ int bg_state(const LmArgs &g, int q) { return min(max(q, 0), g.S - 1); }

// the arcs of state s: [lo, hi) within [0, A)
__device__ __forceinline__ void bg_arcs(const LmArgs &g, int s, int &lo, int &hi) {
    lo = hi = 0;
    if (g.A == 0) return;  // (the arc arrays may be NULL)
    lo = min(max(g.off[s], 0), g.A);
    hi = min(max(g.off[s + 1], lo), g.A);
}

// the first arc of [lo, hi) whose token is >= v (tokens ascend)
__device__ __forceinline__ int bg_lower(const LmArgs &g, int lo, int hi, int v) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (g.tok[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int bg_find(const LmArgs &g, int s, int v) {  // the arc (s, v), or -1
    int lo, hi;
    bg_arcs(g, s, lo, hi);
    const int a = bg_lower(g, lo, hi, v);
    return a < hi && g.tok[a] == v ? a : -1;
}

// ONE hop of the back-off walk of include/rnnt_lm.h, for the step and the select alike: from state cur != E, hop hops into the
// walk, with the running sum acc (not read at hop 0).  After RNNT_LM_MAX_HOPS hops the walk is at E whatever the graph says.
__device__ __forceinline__ void lm_backoff(const LmArgs &g, int &cur, float &acc, int &hop) {
    const float b = g.bs[cur];
    acc = hop == 0 ? b : acc + b;
    cur = bg_state(g, g.bn[cur]);
    if (++hop == RNNT_LM_MAX_HOPS) cur = g.E;
}

// delta(q, v) of include/rnnt_lm.h -> beta; next: the new state
__device__ __forceinline__ float bg_delta(const LmArgs &g, int q, int v, int blank, int &next) {
    next = q;
    if (v == blank) return 0.f;
    int cur = q, hop = 0;
    float acc = 0.f;
    for (;;) {  // (at most RNNT_LM_MAX_HOPS + 1 rounds: lm_backoff ends at E)
        const int a = bg_find(g, cur, v);
        if (a >= 0) {
            next = bg_state(g, g.nxt[a]);
            return hop == 0 ? g.sc[a] : acc + g.sc[a];
        }
        if (cur == g.E) {
            next = g.E;
            return hop == 0 ? g.unk : acc + g.unk;
        }
        lm_backoff(g, cur, acc, hop);
    }
}

#define BEAM_STEP_KERNEL beam_step_lm_kernel
#define BEAM_STEP_BIAS 2
#include "beam_step_body.h"
#undef BEAM_STEP_KERNEL
#undef BEAM_STEP_BIAS

#define BEAM_SELECT_KERNEL beam_select_lm_kernel
#define BEAM_SELECT_TIMED 0
#define BEAM_SELECT_BIAS 2
#include "beam_select_body.h"
#undef BEAM_SELECT_KERNEL
#undef BEAM_SELECT_TIMED
#define BEAM_SELECT_KERNEL beam_select_timed_lm_kernel
#define BEAM_SELECT_TIMED 1
#include "beam_select_body.h"
#undef BEAM_SELECT_KERNEL
#undef BEAM_SELECT_TIMED
#undef BEAM_SELECT_BIAS

template <int DT>
static hipError_t launch_beam_step_lm_dt(const BeamArgs &a, const LmArgs &bg, size_t shm, hipStream_t s) {
    const hipError_t e = set_lds(beam_step_lm_kernel<DT>, shm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(beam_step_lm_kernel<DT>, dim3(a.g.NS, (a.R + 31) / 32), dim3(kGrWaves * 64), shm, s, a, bg);
    return hipGetLastError();
}

// the LM step (include/rnnt_lm.h): graph checked by the caller, lm_states [B K] or NULL
hipError_t launch_beam_step_lm(const float *pred_proj, int *parents, int *emitted, float *topk_logits, int *topk_symbols,
                               float *lse, int J, int V, int B, int T, int K, int N, int blank, int joint_dtype, bool timed,
                               void *workspace, hipStream_t s, const rnntLmGraph *graph, int *lm_states) {
    BeamArgs a = {};
    BeamLayout L;
    if (!beam_bind(a, T, B, K, N, J, V, joint_dtype, timed, workspace, L)) return hipErrorInvalidValue;
    a.g.pred_proj = pred_proj, a.g.blank = blank;
    a.parents = parents, a.emitted = emitted, a.topl = topk_logits, a.tops = topk_symbols, a.lse = lse;
    LmArgs bg = {};
    bg.off = graph->arc_offsets, bg.tok = graph->arc_tokens, bg.nxt = graph->arc_next, bg.sc = graph->arc_score;
    bg.bn = graph->backoff_next, bg.bs = graph->backoff_score, bg.states = lm_states;
    bg.S = graph->num_states, bg.A = graph->num_arcs, bg.unk = graph->unk_score;
    bg.E = graph->empty_state < 0 ? 0 : graph->empty_state >= bg.S ? bg.S - 1 : graph->empty_state;
    hipError_t e;
    const size_t shm = (size_t)J * 32 * sizeof(gf16) * (L.DT == 1 ? 1 : 2);
    if (L.DT == 1) e = launch_beam_step_lm_dt<1>(a, bg, shm, s);
    else if (L.DT == 0) e = launch_beam_step_lm_dt<0>(a, bg, shm, s);
    else e = launch_beam_step_lm_dt<2>(a, bg, shm, s);
    if (e != hipSuccess) return e;
    if (timed) hipLaunchKernelGGL(beam_select_timed_lm_kernel, dim3(B), dim3(256), 0, s, a, bg);
    else hipLaunchKernelGGL(beam_select_lm_kernel, dim3(B), dim3(256), 0, s, a, bg);
    return hipGetLastError();
}

}  // namespace rnnt
