// rnnt_tdtalign_kernels.hip -- forced alignment on the token-and-duration (TDT) lattice: the maximum-probability path among those
// compute_rnnt_loss_tdt sums over (include/rnnt_tdt_align.h; rnnt_tdtalign.h for the lattice and the workspace).
//
//   tdtalign_cells_kernel<L, VEC>   one pass over a slab of logits: per live cell the two log-softmax normalisers (tokens [0, V),
//                                   durations [V, V + D); f32, online max / sum, L lanes per cell), stored as the 2 D edge weights
//                                   wb_i, wl_i (sigma folded in) on skewed rows.  The cell body of tdt_cells_kernel
//                                   (rnnt_tdt_kernels.hip) on the chunk-to-lane map, the chunk load, the merge, the cell
//                                   decomposition and the lane dispatch of rnnt_align_parts.h, which the standard and the modified
//                                   aligner use too; the two-accumulator loop is its own.  HBM-bound.
//   tdtalign_path_kernel<MAXUP>     one workgroup of Up threads per utterance: the max-plus sweep over the skewed rows n = t + u
//                                   (one lattice column per thread, the last dmax + 2 rows of v in an LDS ring, one barrier per row,
//                                   the weights of the next two rows in flight), one decision byte per node, then the back-trace over
//                                   windows of decision bytes staged in LDS and the four outputs.  Another algorithm than the
//                                   bit-lattice sweeps of the other two aligners: it shares nothing with them.
//
// Every sum has an order fixed by V + D alone in the cell pass and every maximum an order fixed by the duration set in the sweep: an
// utterance's outputs do not depend on the batch around it, on how the frames were cut into slabs nor on the load route.
#include "rnnt_align_parts.h"
#include "rnnt_tdtalign.h"

namespace rnnt {

constexpr int kTdtAlignRing = kTdtAlignMaxDuration + 2;  // rows n - dmax - 1 ... n
constexpr int kTdtAlignNone = 0xFF;                      // the decision code of a node nothing arrives at
constexpr int kWinRows = 64, kWinCols = 64;              // the back-trace's window of decision bytes

// ---------------------------------------------------------------------------------------------
// Cell pass: the chunk-to-lane map, the chunk load and the merge of rnnt_align_parts.h over the V + D logits of a cell, with a running
// (max, sum of exp(x - max)) for the tokens and one for the durations -- this file's own loop, since a chunk may straddle the
// boundary between the two.
// ---------------------------------------------------------------------------------------------
template <int L, bool VEC>
__global__ void __launch_bounds__(256) tdtalign_cells_kernel(const TdtAlignParams p) {
    const int j = threadIdx.x % L;
    if (blockIdx.x == 0 && threadIdx.x == 0) *p.sigma_slot = p.sigma;  // (every slab's call writes the same value)
    AlignCell q;
    if (!align_cell_of<L>(p, q)) return;
    const int b = q.b, t = q.t, u = q.u;

    const int V = p.V, D = p.D, R = V + D;
    const float *row = p.acts + (size_t)q.c * (size_t)R;
    const int chunks = (R + 3) >> 2;
    float mv = kAlignNegInit, sv = 0.0f, md = kAlignNegInit, sd = 0.0f;
#pragma unroll 2
    for (int ch = j; ch < chunks; ch += L) {
        const int i = 4 * ch;
        const float4 x4 = align_load_chunk<VEC>(row, ch, R);
        const float x[4] = {x4.x, x4.y, x4.z, x4.w};
        float nv = mv, nd = md;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool tok = i + k < V;
            nv = tok ? fmaxf(nv, x[k]) : nv;
            nd = tok ? nd : fmaxf(nd, x[k]);
        }
        float ev = 0.0f, ed = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool tok = i + k < V;
            const float e = __expf(x[k] - (tok ? nv : nd));  // (the padding: exp(-inf) = 0)
            ev += tok ? e : 0.0f;
            ed += tok ? 0.0f : e;
        }
        sv = sv * __expf(mv - nv) + ev;
        sd = sd * __expf(md - nd) + ed;
        mv = nv, md = nd;
    }
#pragma unroll
    for (int off = L / 2; off >= 1; off >>= 1) {
        align_merge(mv, sv, j, off);
        align_merge(md, sd, j, off);
    }
    const float lseV = mv + __logf(sv), lseD = md + __logf(sd);
    // the 2 + D logits the weights need are read again here (the lines are in cache): which lane holds them depends on V, the blank
    // and the label
    const float lpb = (row[p.blank] - lseV) - p.sigma;
    float lpl = 0.0f;
    if (u < q.Ub) lpl = (row[align_label(p, b, u, V)] - lseV) - p.sigma;
    const size_t plane = (size_t)p.N * (size_t)p.Up;
    float *w = p.w + (size_t)b * (size_t)(2 * D) * plane + (size_t)(t + u) * (size_t)p.Up + u;
    for (int i = j; i < D; i += L) {
        const float ld = row[V + i] - lseD;
        w[(size_t)i * plane] = lpb + ld;
        w[(size_t)(D + i) * plane] = lpl + ld;
    }
}

hipError_t launch_tdtalign_cells(const TdtAlignParams &p, hipStream_t s) {
    const int R = p.V + p.D;
    const bool vec = (R % 4 == 0) && (((uintptr_t)p.acts & 15) == 0);
    return dispatch_cell_lanes((R + 3) / 4, [&](auto L) {
        constexpr int kL = decltype(L)::value;
        if (vec)
            hipLaunchKernelGGL((tdtalign_cells_kernel<kL, true>), dim3(align_cells_grid(p, kL)), dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((tdtalign_cells_kernel<kL, false>), dim3(align_cells_grid(p, kL)), dim3(256), 0, s, p);
        return hipGetLastError();
    });
}

// ---------------------------------------------------------------------------------------------
// Sweep + back-trace.  Thread u owns lattice column u; step n visits the nodes (n - u, u).  Row n of v goes to slot n % kTdtAlignRing
// of the LDS ring; a step reads the slots of rows n - 1 ... n - (dmax + 1), its own column for the blank arrivals and the column
// below for the label arrivals, and writes its own slot, which held row n - kTdtAlignRing: the barrier at the end of a step orders
// this step's writes before the next step's reads AND the previous step's reads before this step's writes to the slot they no longer
// need.  An edge that does not exist gets the weight -inf WITHOUT a load, so what the cell pass never wrote enters no addition, and
// its candidate (-inf) never replaces an incumbent.  Per candidate the work is one float64 add and one compare.
// ---------------------------------------------------------------------------------------------
struct TdtAlignWeights {
    float wb[kTdtAlignMaxD], wl[kTdtAlignMaxD];
};

// the weights of the edges INTO node (n - u, u): those of its source cells (n - d_i - u, u) and (n - d_i - u, u - 1)
__device__ __forceinline__ void tdtalign_load(TdtAlignWeights &x, const TdtAlignParams &p, const float *w, const int n, const int u,
                                              const int Tb, const int Ub) {
    const int t = n - u, D = p.D;
    const size_t plane = (size_t)p.N * (size_t)p.Up;
    const bool node = u <= Ub && t >= 0 && (t < Tb || (t == Tb && u == Ub));
#pragma unroll
    for (int i = 0; i < kTdtAlignMaxD; ++i) {
        x.wb[i] = x.wl[i] = -INFINITY;
        if (i < D) {
            const int d = p.dur[i];
            if (node && d > 0 && t - d >= 0) x.wb[i] = w[(size_t)i * plane + (size_t)(n - d) * (size_t)p.Up + u];
            if (node && u >= 1 && t < Tb && t - d >= 0) x.wl[i] = w[(size_t)(D + i) * plane + (size_t)(n - d - 1) * (size_t)p.Up + u - 1];
        }
    }
}

template <int MAXUP>
__global__ void __launch_bounds__(MAXUP) tdtalign_path_kernel(const TdtAlignParams p) {
    static_assert(kTdtAlignRing * MAXUP * sizeof(double) >= kWinRows * kWinCols, "the window reuses the ring");
    __shared__ double ring[kTdtAlignRing * MAXUP];  // a launch of Up <= MAXUP threads uses kTdtAlignRing * Up of it
    __shared__ int fr[MAXUP];                        // emission frame per token, written by the back-trace
    __shared__ uint8_t di[MAXUP];                    // ... and the index of its duration
    __shared__ int pos[3];                           // the back-trace's node between two windows; [2]: a path exists
    const int b = blockIdx.x, u = threadIdx.x;
    int Tb = p.input_lengths[b], Ub = p.label_lengths[b];
    const bool bad = Tb < 1 || Tb > p.T || Ub < 0 || Ub > p.U - 1;
    Tb = min(max(Tb, 1), p.T);
    Ub = min(max(Ub, 0), p.U - 1);
    const int Up = p.Up, D = p.D;
    int *out_frames = p.token_frames + (size_t)b * (p.U - 1);
    int *out_durs = p.token_durations + (size_t)b * (p.U - 1);
    float *out_logp = p.token_logp + (size_t)b * (p.U - 1);

    if (bad) {  // out-of-range lengths: NaN.  The workspace is not read.
        if (u < p.U - 1) {
            out_frames[u] = -1;
            out_durs[u] = -1;
            out_logp[u] = 0.0f;
        }
        if (u == 0) p.scores[b] = __int_as_float(0x7fc00000);
        return;
    }

    const int last = Tb + Ub;  // the terminal's row; last < N
    const size_t plane = (size_t)p.N * (size_t)Up;
    const float *w = p.w + (size_t)b * (size_t)(2 * D) * plane;
    uint8_t *dec = p.dec + (size_t)b * plane;
    const int side = max(u - 1, 0);  // the column of the label arrivals' source

#pragma unroll
    for (int r = 0; r < kTdtAlignRing; ++r) ring[r * Up + u] = -INFINITY;
    fr[u] = 0;
    di[u] = 0;
    __syncthreads();

    TdtAlignWeights cur, nx1, nx2;
    tdtalign_load(cur, p, w, 0, u, Tb, Ub);
    tdtalign_load(nx1, p, w, 1, u, Tb, Ub);  // (last >= 1)
    nx2 = nx1;
    double v = -INFINITY;
    for (int n = 0; n <= last; ++n) {
        if (n + 2 <= last) tdtalign_load(nx2, p, w, n + 2, u, Tb, Ub);  // two rows ahead: in flight under two steps' arithmetic
        v = -INFINITY;
        int code = kTdtAlignNone;
#pragma unroll
        for (int i = 0; i < kTdtAlignMaxD; ++i) {
            if (i < D) {
                const int d = p.dur[i];
                // rows n - d and n - d - 1; before the first row the ring still holds its -inf
                const int rb = (n - d + 2 * kTdtAlignRing) % kTdtAlignRing, rl = (n - d - 1 + 2 * kTdtAlignRing) % kTdtAlignRing;
                const double cb = ring[rb * Up + u] + (double)cur.wb[i];
                const double cl = ring[rl * Up + side] + (double)cur.wl[i];
                if (cb > v) v = cb, code = 2 * i;  // strictly greater: an exact tie keeps the earlier candidate
                if (cl > v) v = cl, code = 2 * i + 1;
            }
        }
        if (n == 0 && u == 0) v = 0.0;  // v(0, 0)
        ring[(n % kTdtAlignRing) * Up + u] = v;
        dec[(size_t)n * (size_t)Up + u] = (uint8_t)code;
        __syncthreads();
        cur = nx1;
        nx1 = nx2;
    }

    // the score: v(T_b, L_b) of the last step; -inf when no path exists
    if (u == Ub) {
        p.scores[b] = (float)v;
        pos[0] = last, pos[1] = Ub, pos[2] = v > -INFINITY;
    }
    __threadfence();  // the decision bytes are read back by other threads below
    __syncthreads();

    // Back-trace: up to T_b + L_b dependent steps, each needing the decision byte of a node known only after the step before.  The
    // workgroup stages a window of kWinRows rows x kWinCols columns whose top right corner holds the current node (columns aligned to
    // 4 bytes) in LDS -- the ring's memory, free now -- and thread 0 walks it until the path leaves the window: a step moves up to
    // dmax + 1 rows and one column, so a window lasts at least kWinRows / (dmax + 1) steps and, on blank-heavy paths, about kWinRows.
    const bool has_path = pos[2] != 0;
    if (has_path) {
        uint32_t *win = reinterpret_cast<uint32_t *>(ring);  // [kWinRows][kWinCols / 4]
        const uint32_t *dec32 = reinterpret_cast<const uint32_t *>(dec);
        int n = pos[0], uu = pos[1];
        while (n > 0) {
            const int r0 = n - (kWinRows - 1), c0 = max(0, (uu | 3) - (kWinCols - 1));  // c0 % 4 == 0, c0 + kWinCols <= Up
            for (int k = u; k < kWinRows * (kWinCols / 4); k += Up) {
                const int row = r0 + k / (kWinCols / 4), cw = k % (kWinCols / 4);
                win[k] = row >= 0 ? dec32[((size_t)row * (size_t)Up + c0) / 4 + cw] : 0xFFFFFFFFu;
            }
            __syncthreads();
            if (u == 0) {
                while (n > 0 && n >= r0 && uu >= c0) {
                    const int cc = uu - c0;
                    const int code = (int)((win[(n - r0) * (kWinCols / 4) + (cc >> 2)] >> (8 * (cc & 3))) & 0xFFu);
                    const int i = code >> 1, label = code & 1;
                    const int d = (int)((p.dur_packed >> (4 * (i & 7))) & 15u);
                    if (i >= D || (label ? uu < 1 : d < 1) || n - d - label < uu - label) {  // not a decision of this lattice: stop
                        n = 0;                                                                // (a node on a best path has one)
                        break;
                    }
                    if (label) {
                        fr[uu - 1] = n - uu - d;  // token uu - 1 is emitted in frame t - d and claims d frames
                        di[uu - 1] = (uint8_t)i;
                    }
                    n -= d + label;
                    uu -= label;
                }
                pos[0] = n, pos[1] = uu;
            }
            __syncthreads();
            n = pos[0], uu = pos[1];
            __syncthreads();  // (pos is rewritten by the next window's walk)
        }
    }
    if (u < p.U - 1) {
        int f = -1, d = -1;
        float l = 0.0f;
        if (has_path && u < Ub) {
            const int i = di[u];
            f = fr[u];
            d = (int)((p.dur_packed >> (4 * i)) & 15u);
            l = w[(size_t)(D + i) * plane + (size_t)(f + u) * (size_t)Up + u] + p.sigma_slot[0];
        }
        out_frames[u] = f;
        out_durs[u] = d;
        out_logp[u] = l;
    }
}

template <int MAXUP>
static hipError_t launch_path_N(const TdtAlignParams &p, hipStream_t s) {
    hipLaunchKernelGGL((tdtalign_path_kernel<MAXUP>), dim3(p.B), dim3(p.Up), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_tdtalign_path(const TdtAlignParams &p, hipStream_t s) {
    // the instantiation sizes the static LDS ring: the smallest that holds the launch's Up threads
    if (p.Up <= 64) return launch_path_N<64>(p, s);
    if (p.Up <= 128) return launch_path_N<128>(p, s);
    if (p.Up <= 256) return launch_path_N<256>(p, s);
    if (p.Up <= 512) return launch_path_N<512>(p, s);
    return launch_path_N<1024>(p, s);
}

}  // namespace rnnt
