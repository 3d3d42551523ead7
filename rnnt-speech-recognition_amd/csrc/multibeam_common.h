// multibeam_common.h -- what the two translation units of the beam search with several symbols per frame share
// (multibeam_kernels.hip: the offline search of include/rnnt_beam_multi.h; tsd_stream_kernels.hip: its stream,
// include/rnnt_beam_multi_stream.h): the kernels' argument block, the workspace layout and its binding.  The including translation
// unit defines rnnt::kBeamMax and rnnt::kHashMul first, as for beam_common.h.
#pragma once
#include "beam_common.h"

namespace rnnt {

struct MultiBeamArgs {
    BeamArgs b;  // K = beam, R = minibatch 2 K rows, N = max_hyp_len; nslot = |A|; slot / tok / parents / emitted over the 2 K rows
    int *nclosed;  // [B] |B|
    int E;         // symbols per frame
    // the timed stream alone (offline: never read).  They stand last, so every field above keeps its place in the kernel arguments
    int *frm;               // [2][B][2 K][N] per token the frame (since the slot's reset) whose joint evaluation appended it
    const int *frame_base;  // [B] frames of the chunks the slot held before this one
};

// ---------------------------------------------------------------------------------------------
// the workspace: BeamLayout's regions over R = B 2K rows (lists of K per row), and |B| per utterance
// ---------------------------------------------------------------------------------------------
struct MultiBeamLayout {
    BeamLayout b;
    size_t nclosed;
};

static bool make_multibeam_layout(int T, int B, int K, int E, int N, int J, int V, int joint_dtype, MultiBeamLayout &M) {
    BeamLayout &L = M.b;
    L.DT = greedy_dt(joint_dtype, J, V);
    if (L.DT < 0 || T <= 0 || B <= 0 || K < 1 || K > kBeamMax || N < 1 || E < 1 || E > 8) return false;
    if ((long long)B * 2 * K > 1024) return false;  // (the prediction network's rows)
    if ((unsigned long long)B * T * J >= (1ull << 31) || 4ull * B * K * N >= (1ull << 31)) return false;
    if ((unsigned long long)T * (E + 1) >= (1ull << 31)) return false;  // (the step counter)
    L.NC = (V + 31) / 32;
    L.NS = (L.NC + kGrWaves - 1) / kGrWaves;
    const size_t R = (size_t)B * 2 * K;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    L.st = take((size_t)B * sizeof(GreedyState));
    L.slot = take(R * sizeof(BeamSlot));
    L.nslot = take((size_t)B * sizeof(int));
    M.nclosed = take((size_t)B * sizeof(int));
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
    L.tt = off;
    L.total = off;
    return true;
}

static bool multibeam_bind(MultiBeamArgs &m, int T, int B, int K, int E, int N, int J, int V, int joint_dtype, void *workspace,
                           MultiBeamLayout &M) {
    if (!make_multibeam_layout(T, B, K, E, N, J, V, joint_dtype, M)) return false;
    const BeamLayout &L = M.b;
    char *ws = (char *)workspace;
    BeamArgs &a = m.b;
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
    a.tt = nullptr;
    a.K = K, a.R = B * 2 * K, a.N = N;
    m.nclosed = (int *)(ws + M.nclosed);
    m.E = E;
    return true;
}

}  // namespace rnnt
