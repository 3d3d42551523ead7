// rnnt_pruned_joint.h -- the fused joint on the pruned band (include/rnnt_pruned_joint.h): workspace layout and launchers of
// rnnt_pruned_joint_kernels.hip.  The lattice is rnnt_pruned.h's: its layout is the first part of this workspace and its sweep
// launcher (rnnt_pruned_kernels.hip, linked unchanged) runs on it.
//
// Rows are band slots: row (b, t, s) is lattice cell (t, u), u = sb[b][t] + s, PRESENT iff t < T_b, 0 <= u <= L_b.  The kernels
// work on tiles of 32 consecutive slots of ONE utterance; the logits of a tile exist 32 columns at a time, in registers and LDS.
//
// Workspace, a function of (maxT, s_range, minibatch, joint_size) alone:
//   band    PrunedLayout   lp / lse (written by the forward cell kernel for present slots), alpha / edge / lnP (by the sweeps)
//   lse_lo  f32 [B T S]     the low part of the softmax denominator: lse = band.lse + lse_lo (present slots)
//   dz      f32 [B T S][J]  d cost / d (enc_proj + pred_proj) per PRESENT slot, cost_scale applied; absent slots are never
//                           written and never read (the reductions repeat the range test)
//   w2max   u32 [64]        per-block abs-max bit patterns of W2 (rewritten by every call)
//   wpart   f32 [J][8192]   the dW2 partial sums: R row chunks x J x (V rounded up to 32), R = min(256, 8192 / that) >= 1
//   bpart   f32 [8192]      the db2 partial sums: R x (V rounded up to 32)
// Everything a kernel reads was written by a kernel in front of it: the workspace may hold anything on entry.
#pragma once
#include "rnnt_pruned.h"

namespace rnnt {

constexpr int kPJRows = 32;        // band slots per tile: the M of a 32x32x16 MFMA
constexpr int kPJCols = 32;        // vocabulary columns per tile
constexpr int kPJMaxJ = 640;
constexpr int kPJMaxV = 8192;
constexpr int kPJAbsBlocks = 64;   // grid of the abs-max pass over W2 = one entry per lane of a consumer's wavefront
constexpr int kPJPartCols = 8192;  // columns of partial sums the workspace holds (per unit of J)
constexpr int kPJMaxChunks = 256;  // at most this many row chunks in the dW2 pass

struct PrunedJointLayout {
    PrunedLayout band;
    size_t lse_lo, dz, w2max, wpart, bpart, total;
};

inline PrunedJointLayout make_pruned_joint_layout(int T, int S, int B, int J) {
    PrunedJointLayout w;
    w.band = make_pruned_layout(T, S, B);
    size_t off = w.band.total;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = (off + bytes + 255) / 256 * 256;
        return o;
    };
    w.lse_lo = take((size_t)B * T * S * sizeof(float));
    w.dz = take((size_t)B * T * S * J * sizeof(float));
    w.w2max = take(kPJAbsBlocks * sizeof(unsigned));
    w.wpart = take((size_t)J * kPJPartCols * sizeof(float));
    w.bpart = take((size_t)kPJPartCols * sizeof(float));
    w.total = off;
    return w;
}

struct PrunedJointParams {
    PrunedParams band;  // s_begin, labels, lengths, cost_scale, costs, the lattice arrays, B T S U V blank topology fe_lambda
    const float *enc;   // [B][T][J]
    const float *pred;  // [B][U][J]
    const float *W2;    // [J][V]
    const float *b2;    // [V]
    float *d_enc, *d_pred, *dW2, *db2;
    float *lse_lo;
    float *dz;
    unsigned *w2max;
    float *wpart, *bpart;
    int J;
    int tiles_per_utt;    // ceil(T S / 32)
    int vtiles;           // ceil(V / 32)
    int chunks;           // R: row chunks of the dW2 pass
    int tiles_per_chunk;  // ceil(B tiles_per_utt / R)
};

inline void pruned_joint_geometry(PrunedJointParams &p) {
    const long long slots = (long long)p.band.T * p.band.S;
    p.tiles_per_utt = (int)((slots + kPJRows - 1) / kPJRows);
    p.vtiles = (p.band.V + kPJCols - 1) / kPJCols;
    const long long total = (long long)p.band.B * p.tiles_per_utt;
    long long r = kPJPartCols / (p.vtiles * kPJCols);
    if (r > kPJMaxChunks) r = kPJMaxChunks;
    if (r > total) r = total;
    if (r < 1) r = 1;
    p.tiles_per_chunk = (int)((total + r - 1) / r);
    p.chunks = (int)((total + p.tiles_per_chunk - 1) / p.tiles_per_chunk);
}

hipError_t launch_pruned_joint_forward(const PrunedJointParams &p, hipStream_t s);   // W2 abs-max + cell kernel (no sweeps)
// the four gradients; w2max_fresh: launch_pruned_joint_forward ran in front of it in this call (no second abs-max pass)
hipError_t launch_pruned_joint_backward(const PrunedJointParams &p, bool w2max_fresh, hipStream_t s);

}  // namespace rnnt
