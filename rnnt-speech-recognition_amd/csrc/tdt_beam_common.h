// tdt_beam_common.h -- the host side of the TDT beam search's workspace (tdt_beam_kernels.hip): the kernels' argument block, the
// layout and its binding to a workspace pointer.  No kernel lives here.  The including translation unit defines rnnt::kBeamMax and
// rnnt::kHashMul first, as beam_common.h asks (tests/test_tdt_beam.py holds them against beam_kernels.hip's).
//
// The workspace is the beam search's at alphabet_size = R = V + D (beam_common.h make_beam_layout: the state, the slots, the token
// head's partials and slice lists, the double-buffered token rows, the greedy decoder's tables and W2 image over all R columns and,
// timed, the pair rows), followed by the duration head's partials [NS][B K], the raw duration logits [B K][kTdtBeamMaxD] and the
// duration set.  Two words of the beam's layout mean something else here:
//   BeamSlot::pad   the hypothesis's CURSOR, the next frame it reads (the unbiased beam search keeps 0 there)
//   BeamArgs::tt    timed: {emission frame, frames claimed} per token (the beam search: {frame, bits of the log-probability})
// The region BeamArgs::bl (the blank's logit of a hypothesis with a full token row) is not used offline, where a row is never full.
// The stream (tdt_nbest_stream_kernels.hip, include/rnnt_tdt_beam_stream.h) lays the same workspace out with token and pair rows of
// stride N = max_hyp_len (the _n forms below; offline N = T), uses bl, and keeps the cursor relative to the chunk a slot holds.
#pragma once
#include "beam_common.h"
#include "tdt_host.h"

namespace rnnt {

constexpr int kTdtBeamMaxD = 8;  // include/rnnt_tdt.h: 1 <= D <= 8
static_assert(kTdtBeamMaxD == kTdtHostMaxD, "tdt_host.h holds the limit the boundary checks");
// the stream: the word after the duration set (its 256-byte region has room) holds the place of the frame bases, in words past
// this workspace, for the calls that take no enc_width (tdt_stream_kernels.hip does the same)
constexpr int kTdtBeamBaseWord = kTdtBeamMaxD;

struct TdtBeamDurations {
    int d[kTdtBeamMaxD];
};

struct TdtBeamArgs {
    BeamArgs b;  // b.g.V = R, NC / NS over R; g.part_m / part_s, pl / pv: the token head's
    float *dpart_m, *dpart_s;  // [NS][B K] the duration head's partials
    float *dl;                 // [B K][kTdtBeamMaxD] the raw duration logits of the rows that were active
    int *durset;               // [kTdtBeamMaxD]
    int Vt, D;
    float *durl;  // diagnostics: [B K][D] (NULL: not written)
    int *cursors, *hyp_durations;  // results
    const int *tail;  // the stream alone: the end of this workspace; the frame bases [S] are at tail + durset[kTdtBeamBaseWord]
};

struct TdtBeamLayout {
    BeamLayout b;
    size_t dpm, dps, dl, durset, total;
};

// N: the token and pair row stride (offline: T)
static bool make_tdt_beam_layout_n(int T, int B, int K, int N, int J, int Vt, int D, int joint_dtype, bool timed, TdtBeamLayout &L) {
    if (Vt < 2 || D < 1 || D > kTdtBeamMaxD) return false;
    if (!make_beam_layout(T, B, K, N, J, Vt + D, joint_dtype, timed, L.b)) return false;
    size_t off = L.b.total;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    const size_t R = (size_t)B * K;
    L.dpm = take((size_t)L.b.NS * R * sizeof(float));
    L.dps = take((size_t)L.b.NS * R * sizeof(float));
    L.dl = take(R * kTdtBeamMaxD * sizeof(float));
    L.durset = take(kTdtBeamMaxD * sizeof(int));
    L.total = off;
    return true;
}

static bool make_tdt_beam_layout(int T, int B, int K, int J, int Vt, int D, int joint_dtype, bool timed, TdtBeamLayout &L) {
    return make_tdt_beam_layout_n(T, B, K, T, J, Vt, D, joint_dtype, timed, L);
}

static bool tdt_beam_bind_n(TdtBeamArgs &ta, int T, int B, int K, int N, int J, int Vt, int D, int joint_dtype, bool timed,
                            void *workspace, TdtBeamLayout &L) {
    if (!make_tdt_beam_layout_n(T, B, K, N, J, Vt, D, joint_dtype, timed, L)) return false;
    if (!beam_bind(ta.b, T, B, K, N, J, Vt + D, joint_dtype, timed, workspace, L.b)) return false;
    char *ws = (char *)workspace;
    ta.dpart_m = (float *)(ws + L.dpm), ta.dpart_s = (float *)(ws + L.dps);
    ta.dl = (float *)(ws + L.dl), ta.durset = (int *)(ws + L.durset);
    ta.Vt = Vt, ta.D = D;
    return true;
}

static bool tdt_beam_bind(TdtBeamArgs &ta, int T, int B, int K, int J, int Vt, int D, int joint_dtype, bool timed, void *workspace,
                          TdtBeamLayout &L) {
    return tdt_beam_bind_n(ta, T, B, K, T, J, Vt, D, joint_dtype, timed, workspace, L);
}

}  // namespace rnnt
