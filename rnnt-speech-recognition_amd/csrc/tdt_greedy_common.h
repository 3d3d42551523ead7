// tdt_greedy_common.h -- what the translation units of the TDT greedy decoders share (tdt_greedy_kernels.hip: the batched decoder;
// tdt_stream_kernels.hip: the stream over slots, whose own regions follow this layout): the arguments of the step and update
// kernels, the workspace layout and its binding to a workspace pointer, and the update kernel's body.  As greedy_common.h: no
// kernel lives here.  tdt_greedy_step_kernel<DT> lives in tdt_greedy_kernels.hip alone; launch_tdt_greedy_step_kernel launches it
// for the other translation unit.
#pragma once
#include "rnnt_decode.h"
#include "greedy_common.h"
#include "tdt_host.h"

#include <limits.h>
#include <math.h>

namespace rnnt {

constexpr int kTdtGreedyMaxD = 8;
static_assert(kTdtGreedyMaxD == kTdtHostMaxD, "tdt_host.h holds the limit the boundary checks");
constexpr int kTdtStreamBaseWord = kTdtGreedyMaxD;  // durset[this]: where the stream's frame bases lie (tdt_stream_kernels.hip)

struct TdtDurations {
    int d[kTdtGreedyMaxD];
};

struct TdtGreedyArgs {
    GreedyArgs g;  // V = R = Vt + D, NC / NS over R; part_m / part_s / part_i: the token head's partials
    float *dpart_m, *dpart_s;  // [NS][B] the duration head's partials
    int *dpart_i;
    int *durset;  // [kTdtGreedyMaxD] the duration set, then one word the stream keeps (kTdtStreamBaseWord)
    int Vt, D;
};

struct TdtGreedyLayout {
    GreedyLayout g;
    size_t dpm, dps, dpi, durset, total;
};

static bool make_tdt_greedy_layout(int T, int B, int J, int Vt, int D, int joint_dtype, TdtGreedyLayout &L) {
    if (Vt < 2 || D < 1 || D > kTdtGreedyMaxD) return false;
    if (!make_greedy_layout(T, B, J, Vt + D, joint_dtype, L.g)) return false;
    size_t off = L.g.total;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    L.dpm = take((size_t)L.g.NS * B * sizeof(float));
    L.dps = take((size_t)L.g.NS * B * sizeof(float));
    L.dpi = take((size_t)L.g.NS * B * sizeof(int));
    L.durset = take((kTdtGreedyMaxD + 1) * sizeof(int));  // (+ the stream's word: the sizes are what they were, 256 bytes)
    L.total = off;
    return true;
}

static void tdt_greedy_bind(TdtGreedyArgs &ta, const TdtGreedyLayout &L, void *workspace) {
    char *ws = (char *)workspace;
    greedy_bind(ta.g, L.g, workspace);
    ta.dpart_m = (float *)(ws + L.dpm), ta.dpart_s = (float *)(ws + L.dps), ta.dpart_i = (int *)(ws + L.dpi);
    ta.durset = (int *)(ws + L.durset);
}

// tdt_greedy_kernels.hip: tdt_greedy_step_kernel<DT> alone on a bound ta (DT: L.g.DT), for a caller with an update kernel of its own
hipError_t launch_tdt_greedy_step_kernel(const TdtGreedyArgs &ta, int DT, hipStream_t s);

__device__ __forceinline__ bool tg_live(const GreedyState &s, const int max_hyp_len) {
    return !s.done && s.n < min(s.maxsym, max_hyp_len);  // (a full hyps buffer pauses a hypothesis)
}

// the NS partials of hypothesis b in slice order -> argmax (lowest index on ties), max, logsumexp in float64
__device__ __forceinline__ void tg_head(const float *pm, const float *ps, const int *pi, const int NS, const int B, const int b, float &M,
                                        int &k, double &lse) {
    M = -INFINITY, k = INT_MAX;
    for (int q = 0; q < NS; ++q) {
        const float m = pm[(size_t)q * B + b];
        const int i = pi[(size_t)q * B + b];
        if (m > M || (m == M && i < k)) M = m, k = i;
    }
    double S = 0.0;
    for (int q = 0; q < NS; ++q) {
        const float s = ps[(size_t)q * B + b];
        if (s > 0.f) S += (double)s * exp((double)pm[(size_t)q * B + b] - (double)M);
    }
    lse = (double)M + log(S);
}

// update: one workgroup of 256 threads over all hypotheses.  BASED: hyp_frames counts from frame_base[b] (the stream: the frames
// of the chunks the slot has left behind); otherwise frame_base is not read.
template <bool BASED>
__device__ __forceinline__ void tdt_greedy_update_body(const TdtGreedyArgs &ta, const int *frame_base) {
    const GreedyArgs &a = ta.g;
    bool running = false, paused = false;
    for (int b = threadIdx.x; b < a.B; b += 256) {
        GreedyState s = a.st[b];
        int em = -1;
        if (tg_live(s, a.max_hyp_len)) {
            float M, Md;
            int k, i;
            double lse, lsed;
            tg_head(a.part_m, a.part_s, a.part_i, a.NS, a.B, b, M, k, lse);
            tg_head(ta.dpart_m, ta.dpart_s, ta.dpart_i, a.NS, a.B, b, Md, i, lsed);
            if (a.stats) {
                float *st = a.stats + 4 * (size_t)b;
                st[0] = M, st[1] = (float)lse, st[2] = Md, st[3] = (float)lsed;
            }
            const double lp = ((double)M - lse) + ((double)Md - lsed);
            s.score += lp;
            int d = (i >= 0 && i < ta.D) ? ta.durset[i] : 1;  // (a duration head without a finite logit: d = 1)
            if (k == a.blank || k < 0 || k >= ta.Vt) {  // blank (or no finite token logit at all)
                if (d == 0) d = 1;
            } else {
                const size_t o = (size_t)b * a.max_hyp_len + s.n;
                a.hyps[o] = k;
                if (a.hyp_frames) {  // (s.t: the frame of this decision, before the state moves on)
                    a.hyp_frames[o] = BASED ? frame_base[b] + s.t : s.t;
                    a.hyp_logp[o] = (float)lp;
                }
                s.n += 1, s.nf += 1, em = k;
                if (d == 0 && s.nf >= s.cap) d = 1;
            }
            if (d > 0) s.nf = 0;
            s.t += d;  // (the last jump may pass Tb)
            if (s.t >= s.Tb || s.n >= s.maxsym) s.done = 1;
            a.st[b] = s;
        }
        a.emitted[b] = em;
        a.hyp_lengths[b] = s.n;
        a.scores[b] = (float)s.score;
        if (!s.done) {
            if (s.n < a.max_hyp_len) running = true;
            else paused = true;
        }
    }
    const int any_running = __syncthreads_or(running), any_paused = __syncthreads_or(paused);
    if (threadIdx.x == 0) a.all_done[0] = any_running ? 0 : (any_paused ? 2 : 1);
}

}  // namespace rnnt
