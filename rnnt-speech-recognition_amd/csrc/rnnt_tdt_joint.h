// rnnt_tdt_joint.h -- the fused TDT joint (include/rnnt_tdt_joint.h): workspace layout and launchers of rnnt_tdt_joint_kernels.hip.
// The lattice is rnnt_tdt.h's: its layout is the first part of this workspace and its sweep launcher (rnnt_tdt_kernels.hip, linked
// unchanged) runs on it.
//
// Rows are lattice cells.  The kernels work on tiles of ONE frame t by 32 consecutive columns u0 ... u0 + 31 of ONE utterance
// (CT = ceil(U / 32) column tiles per frame); a row is LIVE iff t < T_b and u <= L_b.  The logits of a tile exist 32 columns of
// the V + D at a time, in registers and LDS.
//
// Workspace, a function of (maxT, maxU, minibatch, num_durations, joint_size) alone:
//   lat       TdtLayout          w / lse (written by the forward cell kernel for live cells), alpha / beta / lnP (by the sweeps)
//   lse_lo    float2 [B][T][U]   the low parts of the two softmax denominators: lse = lat.lse + lse_lo (live cells)
//   occ       f32 [B][T][U][D+2] {g_b, g_l, g_0 ... g_{D-1}} of rnnt_tdt.h at unit cost_scale (live cells; written by the
//                                occupancy pass of every gradient call)
//   encpart   f32 [B][T][CT][J]  column sums of dz over the 32 rows of a tile (cost_scale applied)
//   predpart  f32 [B][NCH][U][J] sums of dz over the frames of a chunk of kTJFrameChunk frames, NCH = ceil(T / kTJFrameChunk)
//   w2max     u32 [64]           per-block abs-max bit patterns of W2 (rewritten by every call)
//   wpart     f32 [J][8192]      the dW2 partial sums: R row chunks x J x (V + D rounded up to 32), R = min(256, 8192 / that) >= 1
//   bpart     f32 [8192]         the db2 partial sums: R x (V + D rounded up to 32)
// dz itself is never stored.  Everything a kernel reads was written by a kernel in front of it: the workspace may hold anything
// on entry.
#pragma once
#include "rnnt_tdt.h"

namespace rnnt {

constexpr int kTJRows = 32;        // lattice columns per tile: the M of a 32x32x16 MFMA
constexpr int kTJCols = 32;        // logit columns per tile
constexpr int kTJMaxJ = 640;
constexpr int kTJMaxR = 8192;      // V + D at most
constexpr int kTJAbsBlocks = 64;   // grid of the abs-max pass over W2 = one entry per lane of a consumer's wavefront
constexpr int kTJPartCols = 8192;  // columns of partial sums the workspace holds (per unit of J)
constexpr int kTJMaxChunks = 256;  // at most this many row chunks in the dW2 pass
constexpr int kTJFrameChunk = 32;  // frames per workgroup of the dh kernel: one d_pred_proj partial per chunk

struct TdtJointLayout {
    TdtLayout lat;
    size_t lse_lo, occ, encpart, predpart, w2max, wpart, bpart, total;
    int CT, NCH;
};

inline TdtJointLayout make_tdt_joint_layout(int T, int U, int B, int D, int J) {
    TdtJointLayout w;
    w.lat = make_tdt_layout(T, U, B, D);
    w.CT = (U + kTJRows - 1) / kTJRows;
    w.NCH = (T + kTJFrameChunk - 1) / kTJFrameChunk;
    size_t off = w.lat.total;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    w.lse_lo = take((size_t)B * T * U * 2 * sizeof(float));
    w.occ = take((size_t)B * T * U * (D + 2) * sizeof(float));
    w.encpart = take((size_t)B * T * w.CT * J * sizeof(float));
    w.predpart = take((size_t)B * w.NCH * U * J * sizeof(float));
    w.w2max = take(kTJAbsBlocks * sizeof(unsigned));
    w.wpart = take((size_t)J * kTJPartCols * sizeof(float));
    w.bpart = take((size_t)kTJPartCols * sizeof(float));
    w.total = off;
    return w;
}

struct TdtJointParams {
    TdtParams lat;      // labels, lengths, cost_scale, costs, the lattice arrays, B T U V D blank Up N dur sigma (acts / grads unused)
    const float *enc;   // [B][T][J]
    const float *pred;  // [B][U][J]
    const float *W2;    // [J][V + D]
    const float *b2;    // [V + D]
    float *d_enc, *d_pred, *dW2, *db2;
    float2 *lse_lo;
    float *occ, *encpart, *predpart;
    unsigned *w2max;
    float *wpart, *bpart;
    int J;
    int R;                // V + D
    int CT, NCH;          // column tiles per frame, frame chunks per utterance
    int vtiles;           // ceil(R / 32)
    int chunks;           // row chunks of the dW2 pass
    int tiles_per_chunk;  // ceil(B T CT / chunks)
};

inline void tdt_joint_geometry(TdtJointParams &p) {
    p.R = p.lat.V + p.lat.D;
    p.CT = (p.lat.U + kTJRows - 1) / kTJRows;
    p.NCH = (p.lat.T + kTJFrameChunk - 1) / kTJFrameChunk;
    p.vtiles = (p.R + kTJCols - 1) / kTJCols;
    const long long total = (long long)p.lat.B * p.lat.T * p.CT;
    long long r = kTJPartCols / (p.vtiles * kTJCols);
    if (r > kTJMaxChunks) r = kTJMaxChunks;
    if (r > total) r = total;
    if (r < 1) r = 1;
    p.tiles_per_chunk = (int)((total + r - 1) / r);
    p.chunks = (int)((total + p.tiles_per_chunk - 1) / p.tiles_per_chunk);
}

hipError_t launch_tdt_joint_forward(const TdtJointParams &p, hipStream_t s);  // W2 abs-max + cell kernel (no sweeps)
// the four gradients; w2max_fresh: launch_tdt_joint_forward ran in front of it in this call (no second abs-max pass)
hipError_t launch_tdt_joint_backward(const TdtJointParams &p, bool w2max_fresh, hipStream_t s);

}  // namespace rnnt
