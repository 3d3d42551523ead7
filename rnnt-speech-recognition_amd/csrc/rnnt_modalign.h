// rnnt_modalign.h -- forced alignment on the modified (one symbol per frame) lattice (include/rnnt_modified_align.h):
// workspace layout and launchers of rnnt_modalign_kernels.hip.
//
// Lattice nodes (t, u), 0 <= t <= T_b, 0 <= u <= L_b; every edge advances the frame:
//   v(t,u) = max(v(t-1,u) + lpb(t-1,u), v(t-1,u-1) + lpl(t-1,u-1)),  score = v(T_b, L_b)
// Row t depends on row t - 1 only: the sweep takes T_b serial steps with every column in flight.
//
// Workspace, Up = the sweep's threads x columns per thread (the geometry of rnnt_align.h):
//   lp    float2 [B][T][Up]    {lpb, lpl} of cell (t, u), row-major, for the live cells inside the band u <= t,
//                              L_b - u <= T_b - t; nothing else is written and nothing else enters a sum
//   bits  u32    [B][NB][Up]   back-pointers: bit (t mod 32) of word [t / 32][u] is set when node (t, u) was reached by its label
//                              arrival, from (t-1, u-1).  NB = blocks of 32 rows, rows 0 ... T.  The sweep writes every column of
//                              the blocks 0 ... T_b / 32 before its back-trace reads them.
// Everything a kernel reads was written by the kernel in front of it: the workspace may hold anything on entry.
#pragma once
#include "rnnt_align.h"

namespace rnnt {

// the layout and the kernel argument are the standard aligner's (its `cells` is the lp above); only NB differs
inline AlignLayout make_modalign_layout(int T, int U, int B) {
    return make_align_layout_nb(T, U, B, T / 32 + 1);  // rows 0 ... T
}

hipError_t launch_modalign_cells(const AlignParams &p, hipStream_t s);
hipError_t launch_modalign_path(const AlignParams &p, hipStream_t s);

}  // namespace rnnt
