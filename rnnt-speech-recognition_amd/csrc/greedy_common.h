// greedy_common.h -- the host side of the greedy workspace, shared by the translation units that work on it (greedy_kernels.hip:
// the greedy decoders; tdt_greedy_kernels.hip: the TDT greedy decoder, whose own regions follow this layout): the layout and
// its binding to a workspace pointer.  No kernel lives here.
#pragma once
#include "rnnt_decode.h"

namespace rnnt {

size_t joint_w2_image_bytes(int J, int V);

struct GreedyLayout {
    size_t st, pm, ps, pi, rowflag, expE, encraw, img, btab, tflag, total;
    int NC, NS, DT;
};

static bool make_greedy_layout(int T, int B, int J, int V, int joint_dtype, GreedyLayout &L) {
    L.DT = greedy_dt(joint_dtype, J, V);
    if (L.DT < 0 || T <= 0 || B <= 0) return false;
    if ((unsigned long long)B * T * J >= (1ull << 31)) return false;
    L.NC = (V + 31) / 32;
    L.NS = (L.NC + kGrWaves - 1) / kGrWaves;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    L.st = take((size_t)B * sizeof(GreedyState));
    L.pm = take((size_t)L.NS * B * sizeof(float));
    L.ps = take((size_t)L.NS * B * sizeof(float));
    L.pi = take((size_t)L.NS * B * sizeof(int));
    L.rowflag = take((size_t)B * T * sizeof(int));
    L.expE = take((size_t)B * T * J * sizeof(float));
    L.encraw = take((size_t)B * T * J * sizeof(float));
    L.img = take(L.DT == 1 ? (size_t)L.NC * 32 * J * sizeof(gf16) : joint_w2_image_bytes(J, V));
    L.btab = take((size_t)L.NC * 32 * sizeof(float));
    L.tflag = take(256 + 1024);  // joint_prep_kernel's flag words + b2s (64 words per tile, up to 4 tiles)
    L.total = off;
    return true;
}

static void greedy_bind(GreedyArgs &a, const GreedyLayout &L, void *workspace) {
    char *ws = (char *)workspace;
    a.st = (GreedyState *)(ws + L.st);
    a.part_m = (float *)(ws + L.pm), a.part_s = (float *)(ws + L.ps), a.part_i = (int *)(ws + L.pi);
    a.rowflag = (int *)(ws + L.rowflag);
    a.expE = (float *)(ws + L.expE), a.encraw = (float *)(ws + L.encraw);
    a.img = (gf16 *)(ws + L.img), a.btab = (float *)(ws + L.btab), a.tflag = (const float *)(ws + L.tflag);
    a.NC = L.NC, a.NS = L.NS;
}

}  // namespace rnnt
