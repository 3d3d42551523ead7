/*
 * include/rnnt.h -- C ABI of libwarprnnt.so, the MI355X-native (gfx950) transducer-loss engine.
 *
 * This is the drop-in boundary for the reference's native op.  The reference
 * (noahchalifour/rnnt-speech-recognition) reaches its loss through
 *     utils/loss.py:6        from warprnnt_tensorflow import rnnt_loss
 *     utils/loss.py:34-35    rnnt_loss(y_pred, y_true, spec_lengths, label_lengths)
 * and builds the library behind it with scripts/build_rnnt.sh:1-13, which compiles the
 * warp-transducer submodule into `libwarprnnt.so` (cmake/warp-rnnt-cmakelist.txt:99,119) and
 * installs this header's namesake (cmake/warp-rnnt-cmakelist.txt:137: include/rnnt.h).  The
 * submodule source is absent from the reference tree, so the entry points below restate the
 * library's published C interface; each one names the reference-side
 * interface it replaces.
 *
 * Ownership: the caller owns every buffer.  The library allocates no device memory and never
 * synchronises the host; all work is enqueued on the caller's HIP stream.
 * Location: this library is device-only.  `loc == RNNT_CPU` is rejected with
 * RNNT_STATUS_INVALID_VALUE -- there is deliberately no CPU fallback inside the product.
 */
#ifndef MI355X_RNNT_H
#define MI355X_RNNT_H

#include <stdbool.h>
#include <stddef.h>

/* The library is built with -fvisibility=hidden: only the entry points declared here are exported. */
#if defined(__GNUC__)
#define RNNT_API __attribute__((visibility("default")))
#else
#define RNNT_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Opaque stand-in for hipStream_t so that C callers need no HIP headers.
 * Replaces the `CUstream stream` member of upstream's rnntOptions. */
typedef struct ihipStream_t *rnntStream_t;

/* Replaces upstream rnntStatus_t (include/rnnt.h of warp-transducer; installed by
 * cmake/warp-rnnt-cmakelist.txt:137).  Values keep upstream's order. */
typedef enum {
    RNNT_STATUS_SUCCESS = 0,
    RNNT_STATUS_MEMOPS_FAILED = 1,
    RNNT_STATUS_INVALID_VALUE = 2,
    RNNT_STATUS_EXECUTION_FAILED = 3,
    RNNT_STATUS_UNKNOWN_ERROR = 4
} rnntStatus_t;

/* Replaces upstream rnntComputeLocation. */
typedef enum { RNNT_CPU = 0, RNNT_GPU = 1 } rnntComputeLocation;

/* Replaces upstream rnntOptions (passed by value). */
typedef struct rnntOptions {
    rnntComputeLocation loc; /* must be RNNT_GPU */
    union {
        unsigned int num_threads; /* ignored (CPU location is not provided) */
        rnntStream_t stream;      /* HIP stream all kernels are enqueued on */
    };
    int blank_label; /* reference never passes it -> op default 0 (utils/vocabulary.py:3-6) */
    int maxT;        /* acts.shape[1] */
    int maxU;        /* acts.shape[2] = L_max + 1 (utils/preprocessing.py:177-183); at most 8192, see below */
    bool batch_first; /* must be true: acts is [B, maxT, maxU, V] row-major (1 byte, as upstream) */
} rnntOptions;

/* Replaces upstream get_warprnnt_version(). */
RNNT_API int get_warprnnt_version(void);

/* Replaces upstream rnntGetStatusString(). */
RNNT_API const char *rnntGetStatusString(rnntStatus_t status);

/* Replaces upstream get_workspace_size(maxT, maxU, minibatch, gpu, &size_bytes).
 * `gpu` must be true.  The size depends on (maxT, maxU, minibatch) only. */
RNNT_API rnntStatus_t get_workspace_size(int maxT, int maxU, int minibatch, bool gpu, size_t *size_bytes);

/* Deliberate limits of this library (upstream has none of them; all are reported as RNNT_STATUS_INVALID_VALUE at
 * enqueue time, never as wrong numbers):
 *   maxU <= 8192       up to 1024 the alpha/beta sweeps keep a whole anti-diagonal in the registers of ONE wavefront
 *                      (64 lanes x up to 16 lattice columns); longer label sequences take a plain multi-wave sweep with
 *                      the previous diagonal in LDS and a barrier per diagonal (same results, much slower per diagonal);
 *                      the fused joint entry points stop at maxU = 1024;
 *   B*maxT*maxU < 2^31 cell indices are 32-bit;
 *   workspace 256-byte aligned.
 * Numerics.  Small vocabularies (alphabet_size <= 60, 16-byte-aligned acts) on lattices of up to 1024 columns run on a
 * LINEAR-domain lattice: edge probabilities, alpha / beta as float32 mantissas times 2^(integer frame per sweep lane and block of
 * 4 or 8 diagonals), exact power-of-two renormalisation -- every rounding is RELATIVE, so the gradients come out 1e-7 ... 4e-6
 * from a float64 evaluation of the same logits (costs 1e-9 ... 5e-6 relative).  Mass that falls more than 126 bits below its
 * frame is flushed; whether that mattered is decided per lattice cell by the gradient pass (what a flush can have cost, times
 * the other side's mass, over the likelihood, must stay below 2^-40) and per utterance by the sweeps (likelihood zero /
 * non-finite, alpha-side vs beta-side likelihood, an edge probability below 2^-100).  An utterance that fails is redone by the
 * LOG-domain kernels, exact for any range, so results never depend on the shortcut: a TEAM of workgroups per utterance (round 5:
 * cell phases split over up to 16 CUs, alpha and beta side by side; one flagged utterance in a B=32 T=600 U=150 batch costs
 * +0.3 ms on a 0.23 ms step -- one workgroup per utterance took +2 ms -- and a batch in which EVERY utterance is handed back
 * 1.2 ms instead of 2.3).
 * N(0,1) logits and trained-like posteriors (one dominant symbol per cell along any monotone alignment) stay on the linear
 * lattice.  Unstructured logits of 4 x N(0,1) sit on the edge at that size (the sweeps shorten their frame blocks from 8 to 4
 * diagonals where the lsm pass saw the mass decay fast; some draws pass the certificate, others -- about a third of the
 * utterances of a batch -- are handed back); from about 5 x N(0,1) on every utterance is.  Larger vocabularies, unaligned
 * tensors, more than 1024 columns, the wide (640 < joint_size <= 704) and the f16 fused joints run on the log-domain kernels
 * throughout; the f32-grade fused joint (joint_dtype 0, joint_size <= 640) runs on the linear lattice since round 5, with the
 * same certificate and the same hand-back (from its parked logits).
 * The log-domain kernels keep alpha / beta as log2 values.  Wherever THIS op uses them (the hand-back, vocabularies above 60
 * symbols, unaligned tensors, more than 1024 columns) the recurrence is carried in float64 registers -- the log2(1 + 2^-|d|) term
 * of a log-add, in (0, 1], on the float32 units -- and only the stored lattice is float32 (residues against an integer offset per
 * block of 8 diagonals and sweep lane / group of 64 columns): a float32 recurrence rounds every log-add at the magnitude of its
 * residue, a random walk that reached 1e-4 ... 5e-4 of gradient error over the ~1,000-step paths of peaked or wide lattices
 * (rounds 1-3; tests/tools/emulate_sweep.py).  The wide f32-grade fused joint (joint_dtype 0, 640 < joint_size <= 704) and the
 * hand-back of the ordinary one use the float64 recurrence as well; the f16 joint (joint_dtype 1: binary16 roundings set its error)
 * keeps the float32 one up to 6 columns per lane (maxU <= 384).
 * Bars, against a float64 evaluation of the same logits, all tested with FIXED bars (tests/test_lin_gpu.py,
 * tests/test_peaky_gpu.py, tests/test_peaky_wide_gpu.py, tests/test_loss_gpu.py; measured values in profiles/r04_accuracy*.json):
 *   costs      within 1e-4 max(1, |cost|) everywhere (measured <= 6e-6);
 *   gradients  within 1e-4 absolute on every input: N(0,1), 4 x N(0,1), 8 x N(0,1) logits and trained-like posteriors, lattices
 *              of up to 8192 columns, every vocabulary size (measured: linear lattice 1e-7 ... 4e-6; log-domain paths 4e-6 at
 *              4 x N(0,1) and 1.1e-5 at 8 x N(0,1) at B=32 T=600 U=150 V=28, up to 4.4e-5 at 8 x N(0,1) on 1000-column lattices,
 *              5.5e-5 at T=1500 U=300 V=1024; 5,000 random shapes up to 1000 columns, half of them at 4 x N(0,1): 3.0e-5).
 * Vocabularies of more than 60 symbols (one lattice cell per wavefront): a cell whose occupancy alpha.beta/L is below 2^-50 gets
 * exactly zero gradients -- every gradient of a cell is bounded by 2 |cost_scale| x its occupancy -- and its logits are not read
 * (the reference's kernel leaves values around 1e-15 there).  The headline path (alphabet_size <= 60) visits every cell.
 * Out-of-range per-utterance lengths (T_b < 1, T_b > maxT, L_b < 0, L_b > maxU-1) are device data and cannot be
 * checked at enqueue time: the kernels clamp them into the tensor (no out-of-bounds access) and report that
 * utterance with a NaN cost and NaN gradients.  Labels outside [0, alphabet_size) are clamped into range. */

/* Replaces upstream compute_rnnt_loss(...): the body of the WarpRNNT TensorFlow op that
 * utils/loss.py:34-35 calls.
 *
 *   acts           device f32 [minibatch, maxT, maxU, alphabet_size]  RAW LOGITS (the log-softmax
 *                  is fused, as in upstream's GPU path; utils/loss.py:29-30 skips it on CUDA builds)
 *   grads          device f32, same shape, or NULL for score-only.  Receives d cost_b / d acts;
 *                  padded cells (t >= T_b or u > L_b) are written as exact zeros, so the caller
 *                  need not pre-zero it.
 *   flat_labels    device i32 [minibatch, maxU-1] (padded rows, as run_rnnt.py:262-263 passes them)
 *   label_lengths  device i32 [minibatch]   L_b
 *   input_lengths  device i32 [minibatch]   T_b (already divided by the time-reduction factor,
 *                  utils/loss.py:31-33)
 *   costs          device f32 [minibatch]   -ln P(y_b | x_b)
 *   workspace      device, >= get_workspace_size() bytes, 256-byte aligned
 *
 * Returns immediately after enqueueing; errors detected at enqueue time are returned, device
 * faults surface on the caller's next stream synchronisation. */
RNNT_API rnntStatus_t compute_rnnt_loss(const float *acts, float *grads, const int *flat_labels,
                               const int *label_lengths, const int *input_lengths,
                               int alphabet_size, int minibatch, float *costs, void *workspace,
                               rnntOptions options);

/* Build-only split of compute_rnnt_loss (no upstream counterpart).  The reference multiplies the
 * op's gradient by the upstream gradient afterwards (the TF binding's registered gradient;
 * run_rnnt.py:278 makes that factor 1/global_batch).  Splitting the call lets an autograd host
 * run the gradient pass only when backward is requested and fold that factor in for free:
 *   compute_rnnt_loss_fwd  = costs + lattice state in `workspace` (reads acts once)
 *   compute_rnnt_loss_bwd  = grads[b] = cost_scale[b] * d cost_b / d acts  (cost_scale NULL = 1),
 *                            from the SAME acts and the workspace left by _fwd.
 * compute_rnnt_loss(acts, grads, ...) == _fwd followed by _bwd(cost_scale = NULL).
 * _bwd may be called more than once per _fwd (an utterance the linear lattice handed back keeps its log-domain state for it).
 *   compute_rnnt_loss_ex   = compute_rnnt_loss with cost_scale folded into grads, in ONE call
 *                            (_fwd followed by _bwd on the caller's stream; nothing else differs). */
RNNT_API rnntStatus_t compute_rnnt_loss_fwd(const float *acts, const int *flat_labels,
                                   const int *label_lengths, const int *input_lengths,
                                   int alphabet_size, int minibatch, float *costs, void *workspace,
                                   rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_loss_bwd(const float *acts, float *grads, const int *flat_labels,
                                   const int *label_lengths, const int *input_lengths,
                                   const float *cost_scale, int alphabet_size, int minibatch,
                                   void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_loss_ex(const float *acts, float *grads, const int *flat_labels,
                                  const int *label_lengths, const int *input_lengths,
                                  const float *cost_scale, int alphabet_size, int minibatch,
                                  float *costs, void *workspace, rnntOptions options);

/* Build-only flag (no upstream counterpart): RNNT_VISIT_ALL switches the occupancy floor OFF -- the gradient kernels then visit
 * every lattice cell / row, as the reference's op and TensorFlow's autodiff do (run_rnnt.py:284), whatever the data.  Where the
 * floor applies (the op at every vocabulary size; the backward of the fused joints below) a cell, or a lattice row of a
 * 32-column tile, whose occupancy alpha.beta/L is at most 2^-50 (the op) / 2^-40 (the fused joints: see get_rnnt_joint_backward_rows)
 * gets exact zeros without its logits being read: results differ from the all-visited ones by less than 2^-44 |cost_scale| per
 * element (the op; the fused joints skip only what is an exact zero already) and run times follow the width of the alignment band.
 * The floor hides no NaN: the forward pass reads every cell, a NaN logit makes the utterance's lattice, cost and occupancies NaN,
 * and a NaN occupancy counts as occupied (tests/test_loss_gpu.py::test_occupancy_floor_and_its_opt_out above 60 symbols,
 * tests/test_tile_floor_gpu.py at and below).  The range certificate of the linear lattice still runs on every skipped cell.  The flag is there for
 * parity debugging and for timing that does not depend on the data (bench.py reports both).
 *   compute_rnnt_loss_flags = compute_rnnt_loss_ex with `flags` (0 or RNNT_VISIT_ALL);  costs == NULL: the gradient pass alone
 *   (compute_rnnt_loss_bwd), grads == NULL: the forward alone.
 *   The fused-joint entry points take the same bit OR-ed into joint_dtype (joint_dtype | RNNT_VISIT_ALL). */
#define RNNT_VISIT_ALL 0x100
RNNT_API rnntStatus_t compute_rnnt_loss_flags(const float *acts, float *grads, const int *flat_labels,
                                     const int *label_lengths, const int *input_lengths,
                                     const float *cost_scale, int alphabet_size, int minibatch,
                                     float *costs, void *workspace, rnntOptions options, unsigned int flags);

/* Build-only extension (no upstream counterpart): FastEmit regularisation of the GRADIENTS (Yu et al. 2021, "FastEmit: Low-latency
 * Streaming ASR with Sequence-level Emission Regularization"): the gradient that flows through the lattice's label edges is scaled
 * by 1 + fastemit_lambda, which trains a streaming model to emit its tokens sooner.  With, per valid cell,
 *   e_b = alpha(t,u) p(blank) beta(t+1,u) / L  (the terminal cell: alpha p(blank) / L),  e_l = alpha(t,u) p(y_u) beta(t,u+1) / L,
 *   occ = e_b + e_l = alpha beta / L,
 *   grads[t,u,v] = cost_scale[b] ( (occ + lambda e_l) softmax(x[t,u,:])[v] - [v == blank] e_b - [v == y_u] (1 + lambda) e_l )
 * -- the chain rule through the fused log-softmax with d cost / d lp[blank] unchanged and d cost / d lp[y_u] times 1 + lambda, so
 * every cell's gradients still sum to zero over v.  The costs stay the plain -ln P; lambda = 0 is compute_rnnt_loss_flags, launched
 * through the same kernels, bit for bit; padded cells stay exact zeros.
 * fastemit_lambda must be finite and in [0, 1] (typical: 1e-3 ... 1e-2); anything else returns RNNT_STATUS_INVALID_VALUE before
 * anything is enqueued.  The upper limit keeps the bounds above as they are written: every gradient of a cell is bounded by
 * (1 + lambda) |cost_scale| x its occupancy (the softmax term by (occ + lambda e_l) p_v, the corrections by e_b <= occ and
 * (1 + lambda) e_l, and a difference of two non-negative terms by the larger), i.e. by 2 |cost_scale| x occupancy for lambda <= 1:
 * the occupancy floors of the op (2^-50) and of the fused joints (2^-40) skip only what they skipped before, and the f32-grade
 * joint's power-of-two dlogits scale keeps |S dl| <= 2^14.  The f16 joint, whose scale is sized to S |cost_scale| <= 2^14 exactly,
 * halves it when lambda > 0 (S |cost_scale| <= 2^13), so that S |dl| <= 2^14 x occupancy holds for it too.
 *   compute_rnnt_loss_fastemit = compute_rnnt_loss_flags (same NULL conventions: costs == NULL runs the gradient pass alone,
 *   grads == NULL the forward alone) with the trailing fastemit_lambda.  The fused joints: compute_rnnt_joint_loss_bwd_fastemit /
 *   compute_rnnt_joint_net_loss_bwd_fastemit below. */
RNNT_API rnntStatus_t compute_rnnt_loss_fastemit(const float *acts, float *grads, const int *flat_labels,
                                        const int *label_lengths, const int *input_lengths,
                                        const float *cost_scale, int alphabet_size, int minibatch,
                                        float *costs, void *workspace, rnntOptions options, unsigned int flags,
                                        float fastemit_lambda);

/* ------------------------------------------------------------------------------------------
 * Build-only extension (no upstream counterpart): the joint network fused with the loss, so the
 * [B,T,U,J] and [B,T,U,V] tensors of model.py:158-166 are never materialised.
 *
 * The first Dense layer is factored exactly:  W1^T(e_t + p_u) + b1 = (W1^T e_t + b1) + W1^T p_u,
 * so the caller passes the two small projections
 *   enc_proj   device f32 [B, maxT, J]   = enc  @ W1 + b1   (model.py:162-163, bias folded here)
 *   pred_proj  device f32 [B, maxU, J]   = pred @ W1
 * and the kernels evaluate  logits[b,t,u,:] = tanh(enc_proj[b,t,:] + pred_proj[b,u,:]) @ W2 + b2
 * (model.py:162-166) tile by tile on the matrix cores.
 *
 *   W2 [J, V], b2 [V]            device f32 (model.py:165-166)
 *   cost_scale                   device f32 [B] or NULL (=1): upstream gradient of each cost, e.g.
 *                                1/global_batch (run_rnnt.py:278)
 *   d_enc_proj [B,maxT,J], d_pred_proj [B,maxU,J], dW2 [J,V], db2 [V]
 *                                device f32 outputs: gradients of sum_b cost_scale[b]*cost_b.
 *                                Fully overwritten.  May all be NULL for score-only.
 *   joint_dtype                  arithmetic of the J x V products.
 *                                0 = f32-grade products (operands split into binary16 hi + lo parts, three f16 MFMAs per product, f32
 *                                    accumulation).  W2 enters the products scaled by the power of two that puts max |W2| into
 *                                    [2^13, 2^14): any finite magnitude is taken (round 5; before, weights beyond binary16's
 *                                    65504 switched the call to plain f32 MFMA kernels), weights within 2^-13 of the largest
 *                                    keep 22 significand bits, smaller ones an absolute error of 2^-38 max |W2|.  Small
 *                                    vocabularies: alphabet_size <= 128 for joint_size a multiple of 64 up to 640 (vocabulary
 *                                    tiles of 32 symbols, one pass of the kernels per tile; <= 32 is the reference's character
 *                                    set), alphabet_size <= 32 for joint_size 704.
 *                                    The backward (joint_size <= 640) does not visit lattice rows, in tiles of 32 columns, whose
 *                                    cells all have an occupancy alpha.beta/L below 2^-40: those cells get exactly zero where the
 *                                    reference leaves ~1e-12 (get_rnnt_joint_backward_rows below: the bound, and how many rows a
 *                                    call visited); its run time follows the width of the alignment band.
 *                                1 = f16 MFMA, larger vocabularies: alphabet_size a multiple of 128 (128 ... 8192),
 *                                    joint_size a multiple of 128 (128 ... 640).  h = tanh(.) and W2 are rounded to binary16
 *                                    (round-to-nearest-even) before the products, accumulation is f32; the loss gradient
 *                                    w.r.t. the logits is scaled by 2^(14 - ceil(log2 max|cost_scale|)) and rounded to
 *                                    binary16 before dh = dl.W2^T and dW2 = h^T.dl (the backward skips lattice rows without mass,
 *                                    as joint_dtype 0 does -- groups of four rows of a 32-column tile here, below an occupancy of
 *                                    2^-40: every binary16 dlogits value of such a row is an exact zero already, the scaled
 *                                    gradient being below 2^-26 there; RNNT_VISIT_ALL switches that off).  The lattice (log-softmax, alpha,
 *                                    beta, costs) stays f32.  A forward pass that knows a backward pass follows (the
 *                                    one-call entry with gradients, or _fwd) PARKS the softmax numerators in the workspace:
 *                                    per (cell, 32-symbol chunk) 2^(x log2 e - R) rounded to binary16, R = the integer at or
 *                                    above the chunk's largest x log2 e (|R| <= 30000); the backward pass multiplies them back
 *                                    with one f32 factor per chunk, in place (one more binary16 rounding of occupancy x softmax;
 *                                    the blank and label columns come from the unrounded f32 edge logits).  A SECOND _bwd
 *                                    call on the same workspace finds the parked values consumed and recomputes the
 *                                    logits instead (one rounding less; results differ by binary16 rounding noise).
 *                                    Counterpart of the reference's `mixed_float16` policy (run_rnnt.py:96-99); oracle:
 *                                    oracle/rnnt_oracle.py joint_loss_and_grads_f16 (parked=True / False).
 *                                Either value may carry RNNT_VISIT_ALL (above): joint_dtype = 0 | RNNT_VISIT_ALL makes the backward
 *                                visit every lattice row.
 *                                Any other (joint_dtype, shape) combination returns RNNT_STATUS_INVALID_VALUE -- checked before
 *                                anything is enqueued, in every entry point that takes joint_dtype.
 *                                get_joint_workspace_size needs no dtype: where both arithmetic types take the shape (alphabet_size 128)
 *                                it returns the larger of the two layouts.
 * Both: maxU <= 1024; enc_proj, pred_proj (and b2 for joint_dtype 1) 16-byte aligned.
 * compute_rnnt_joint_loss      = costs and all four gradients in one call
 * compute_rnnt_joint_loss_fwd  = costs (+ the state a _bwd call needs, kept in `workspace`); for costs ONLY (evaluation) call
 *                                compute_rnnt_joint_loss with NULL gradient pointers -- it leaves nothing for a backward pass
 * compute_rnnt_joint_loss_bwd  = the gradients, from the same inputs and that workspace (autograd split,
 *                                as compute_rnnt_loss_fwd/_bwd); may be called more than once per _fwd
 */
RNNT_API rnntStatus_t get_joint_workspace_size(int maxT, int maxU, int minibatch, int joint_size,
                                      int alphabet_size, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_joint_loss(const float *enc_proj, const float *pred_proj,
                                     const float *W2, const float *b2, const int *flat_labels,
                                     const int *label_lengths, const int *input_lengths,
                                     const float *cost_scale, int joint_size, int alphabet_size,
                                     int minibatch, float *costs, float *d_enc_proj,
                                     float *d_pred_proj, float *dW2, float *db2, int joint_dtype,
                                     void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_joint_loss_fwd(const float *enc_proj, const float *pred_proj,
                                         const float *W2, const float *b2, const int *flat_labels,
                                         const int *label_lengths, const int *input_lengths,
                                         int joint_size, int alphabet_size, int minibatch,
                                         float *costs, int joint_dtype, void *workspace,
                                         rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_joint_loss_bwd(const float *enc_proj, const float *pred_proj,
                                         const float *W2, const float *b2, const int *flat_labels,
                                         const int *label_lengths, const int *input_lengths,
                                         const float *cost_scale, int joint_size, int alphabet_size,
                                         int minibatch, float *d_enc_proj, float *d_pred_proj,
                                         float *dW2, float *db2, int joint_dtype, void *workspace,
                                         rnntOptions options);

/* compute_rnnt_joint_loss_bwd with FastEmit (compute_rnnt_loss_fastemit above): the four gradients back-propagated from
 * FastEmit's dlogits.  The forward entry points serve unchanged -- lambda touches only the backward pass -- and the call may follow
 * any _fwd call any number of times, with a different fastemit_lambda each time (joint_dtype 1: the first call consumes the parked
 * values, later ones recompute the logits, as for compute_rnnt_joint_loss_bwd).  fastemit_lambda = 0 is compute_rnnt_joint_loss_bwd. */
RNNT_API rnntStatus_t compute_rnnt_joint_loss_bwd_fastemit(const float *enc_proj, const float *pred_proj,
                                         const float *W2, const float *b2, const int *flat_labels,
                                         const int *label_lengths, const int *input_lengths,
                                         const float *cost_scale, int joint_size, int alphabet_size,
                                         int minibatch, float *d_enc_proj, float *d_pred_proj,
                                         float *dW2, float *db2, int joint_dtype, void *workspace,
                                         rnntOptions options, float fastemit_lambda);

/* Build-only extension: the WHOLE joint network of model.py:158-166 fused with the loss -- the first Dense layer
 * (model.py:162-163) and its backward run inside the library too, on the matrix cores, f32-grade:
 *   enc   device f32 [B, maxT, H]  encoder output        pred  device f32 [B, maxU, H]  prediction-network output
 *   W1 [H, J], b1 [J]   (Keras Dense kernel / bias, model.py:162-163)          W2 [J, V], b2 [V]  (model.py:165-166)
 *   logits[b,t,u,:] = tanh((enc[b,t,:] + pred[b,u,:]) @ W1 + b1) @ W2 + b2, never materialised; the layer is factored exactly
 *   as (enc @ W1 + b1) + pred @ W1 (three GEMMs over B (maxT + maxU) rows with their operands split into binary16 hi + lo
 *   parts, as for joint_dtype 0: csrc/dense_kernels.hip) and the rest is compute_rnnt_joint_loss on those projections.
 *   Precision of those GEMMs: each of enc, pred, W1 and the two projection gradients is kept to 22 significand bits relative to
 *   ITS largest magnitude m, for 2^-49 <= m < 2^77 (the per-tensor power-of-two scale is held within 2^-63 .. 2^63, so that
 *   every product rescales by a normal f32 number).  A tensor with m < 2^-49 -- a pred of 1e-36 throughout, a gradient under a
 *   vanishing cost_scale -- keeps an absolute resolution of 2^-87 and reads as zero below 2^-88; results stay finite.  A tensor
 *   that reaches 2^79 overflows its binary16 image and gives inf / NaN, as a tensor that holds inf or NaN does.
 *   d_enc [B,maxT,H], d_pred [B,maxU,H], dW1 [H,J], db1 [J], dW2 [J,V], db2 [V]: gradients of sum_b cost_scale[b] * cost_b
 *   (all six or none; fully overwritten; padded frames / label positions get exact zeros in d_enc / d_pred).
 * hidden_size a multiple of 32, joint_size a multiple of 64 (both <= 4096), then the (joint_size, alphabet_size, joint_dtype)
 * rules of compute_rnnt_joint_loss; enc, pred, W1, b1 and the four first-layer gradients (d_enc, d_pred, dW1, db1) 16-byte aligned.  workspace: get_joint_net_workspace_size() bytes, 256-byte
 * aligned; _bwd needs the workspace left by _fwd of the same inputs (projections and operand images live there). */
RNNT_API rnntStatus_t get_joint_net_workspace_size(int maxT, int maxU, int minibatch, int hidden_size,
                                                   int joint_size, int alphabet_size, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_joint_net_loss(const float *enc, const float *pred, const float *W1,
                                                  const float *b1, const float *W2, const float *b2,
                                                  const int *flat_labels, const int *label_lengths,
                                                  const int *input_lengths, const float *cost_scale,
                                                  int hidden_size, int joint_size, int alphabet_size,
                                                  int minibatch, float *costs, float *d_enc, float *d_pred,
                                                  float *dW1, float *db1, float *dW2, float *db2,
                                                  int joint_dtype, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_joint_net_loss_fwd(const float *enc, const float *pred, const float *W1,
                                                      const float *b1, const float *W2, const float *b2,
                                                      const int *flat_labels, const int *label_lengths,
                                                      const int *input_lengths, int hidden_size,
                                                      int joint_size, int alphabet_size, int minibatch,
                                                      float *costs, int joint_dtype, void *workspace,
                                                      rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_joint_net_loss_bwd(const float *enc, const float *pred, const float *W1,
                                                      const float *b1, const float *W2, const float *b2,
                                                      const int *flat_labels, const int *label_lengths,
                                                      const int *input_lengths, const float *cost_scale,
                                                      int hidden_size, int joint_size, int alphabet_size,
                                                      int minibatch, float *d_enc, float *d_pred, float *dW1,
                                                      float *db1, float *dW2, float *db2, int joint_dtype,
                                                      void *workspace, rnntOptions options);

/* compute_rnnt_joint_net_loss_bwd with FastEmit (compute_rnnt_loss_fastemit above): all six gradients from FastEmit's dlogits. */
RNNT_API rnntStatus_t compute_rnnt_joint_net_loss_bwd_fastemit(const float *enc, const float *pred, const float *W1,
                                                      const float *b1, const float *W2, const float *b2,
                                                      const int *flat_labels, const int *label_lengths,
                                                      const int *input_lengths, const float *cost_scale,
                                                      int hidden_size, int joint_size, int alphabet_size,
                                                      int minibatch, float *d_enc, float *d_pred, float *dW1,
                                                      float *db1, float *dW2, float *db2, int joint_dtype,
                                                      void *workspace, rnntOptions options, float fastemit_lambda);

/* Build-only extension: the joint network alone, for decoding.  Replaces `joint(model, f, g)` of the reference's greedy
 * decoder (utils/decoding.py:6-18: dense_1 (tanh) and dense_2 on f + g for one lattice cell per step; called at :63-69):
 *   logits[b,t,u,:] = tanh(enc_proj[b,t,:] + pred_proj[b,u,:]) @ W2 + b2        device f32 [minibatch, maxT, maxU, alphabet_size]
 * with enc_proj / pred_proj as for compute_rnnt_joint_loss (the first Dense layer factored, bias folded into enc_proj).
 * It runs the forward kernels of compute_rnnt_joint_loss with the same joint_dtype on a lattice whose every cell is live, so a
 * decoder sees the logits the loss was trained on:
 *   joint_dtype 0  f32-grade split-precision products (the same power-of-two scale of W2): alphabet_size <= 32,
 *                  joint_size a multiple of 64 (<= 704);
 *   joint_dtype 1  operands rounded to binary16, f32 accumulation (the reference's default vocabulary of 4096 word pieces,
 *                  hparams.py:4): alphabet_size a multiple of 128 (128 ... 8192), joint_size a multiple of 128 (128 ... 640); logits 16-byte aligned.
 * maxU <= 1024; a greedy decoder calls it with maxT = maxU = 1 and minibatch = the number of hypotheses.
 * workspace: get_joint_workspace_size(maxT, maxU, minibatch, joint_size, alphabet_size) bytes, 256-byte aligned. */
RNNT_API rnntStatus_t compute_rnnt_joint_logits(const float *enc_proj, const float *pred_proj,
                                                const float *W2, const float *b2, int joint_size,
                                                int alphabet_size, int minibatch, float *logits,
                                                int joint_dtype, void *workspace, rnntOptions options);

/* Diagnostics of the fused joints' backward (joint_dtype 0 at joint_size <= 640; joint_dtype 1 since round 6): how many lattice rows x 32-column tiles the
 * LAST backward on this workspace visited (rows[0]) out of those inside the utterances (rows[1]).  The backward skips a row of a
 * tile when none of its 32 cells has an occupancy alpha.beta/L above 2^-40: every dlogits value of a cell is bounded by
 * 2 |cost_scale| x that occupancy, and both joints hand dlogits to their products as binary16 parts of (power of two <= 2^13 / |cost_scale|) x
 * dlogits -- below 2^-26 in such a row, i.e. exact zeros already: the row adds nothing, its cells get exactly zero where
 * the reference leaves 1e-12's.  How many rows that is depends on the data (unstructured N(0,1) logits on a 600 x 150 lattice: about
 * half; a trained model: most).  Synchronises options.stream.  rows = {-1, -1} where nothing is skipped (the wide joint, 640 < joint_size)
 * and where the workspace does not hold the counts of a backward of THIS shape (fresh, or used by another shape since: the row plan stamps them).
 * The work of a backward call is divided among the workgroups by these counts, deterministically. */
RNNT_API rnntStatus_t get_rnnt_joint_backward_rows(void *workspace, int joint_size, int alphabet_size, int minibatch,
                                                   rnntOptions options, int rows[2]);

/* The same from the encoder / prediction-network outputs: the first Dense layer (model.py:162-163, utils/decoding.py:8,15) runs
 * in the library too (the split-precision GEMMs of compute_rnnt_joint_net_loss), then the joint as above.
 *   enc [minibatch, maxT, hidden_size], pred [minibatch, maxU, hidden_size], W1 [hidden_size, joint_size], b1 [joint_size]
 *   (16-byte aligned; hidden_size a multiple of 32).  workspace: get_joint_net_workspace_size(...) bytes. */
RNNT_API rnntStatus_t compute_rnnt_joint_net_logits(const float *enc, const float *pred, const float *W1, const float *b1,
                                                    const float *W2, const float *b2, int hidden_size, int joint_size,
                                                    int alphabet_size, int minibatch, float *logits, int joint_dtype,
                                                    void *workspace, rnntOptions options);

/* Build-only extension: batched GREEDY DECODING.  Replaces the reference's one-utterance loop (utils/decoding.py:21-108: per
 * encoder frame, emit the joint's argmax until it is the blank) with a decoder over every utterance of a batch at once.  The
 * caller steps the prediction network; the library evaluates the joint for one lattice cell per hypothesis -- its current
 * frame against its prediction-network output -- and does the argmax, the log-softmax of the decision and the state update
 * in the same pass, without writing logits.
 *
 *   enc_proj      device f32 [minibatch, maxT, joint_size] = enc @ W1 + b1 (bias folded, as for compute_rnnt_joint_logits)
 *   pred_proj     device f32 [minibatch, joint_size]       = pred @ W1 of each hypothesis's CURRENT prediction-network output
 *   W2 [joint_size, alphabet_size], b2 [alphabet_size]     device f32 (model.py:165-166)
 *   frame_lengths device i32 [minibatch]   frames of each utterance; clamped into [0, maxT]
 *   max_symbols   device i32 [minibatch] or NULL: symbols each hypothesis may emit at most (negative = 0; NULL = no limit
 *                 beyond max_hyp_len)
 *   max_per_frame symbols per frame at most, then the next frame; <= 0: no cap (the reference's semantics)
 *   options       loc RNNT_GPU, stream, blank_label (the stop symbol, < alphabet_size), maxT; maxU >= 1 (unused).
 *                 The same options for begin and every step of one decode.
 *
 * compute_rnnt_greedy_begin (once per decode) builds the W2 operand image, the e^{2x} tables of enc_proj for every frame and
 * resets every hypothesis: frame 0, no symbols, score 0; done when frame_lengths[b] or max_symbols[b] is 0.  The workspace then
 * holds everything the steps need: enc_proj and W2 may be reused or freed by the caller.
 * compute_rnnt_greedy_step (once per decode step), for every hypothesis b that is not done:
 *   k = argmax_v logits[b, v] (lowest index on ties, as torch.argmax), logits = tanh(enc_proj[b, t_b] + pred_proj[b]) @ W2 + b2;
 *   scores[b] += log_softmax(logits)[k];  k == blank_label: t_b += 1;  else hyps[b, n_b] = k, n_b += 1, and t_b += 1 when
 *   max_per_frame symbols were emitted at this frame;  done when t_b >= frame_lengths[b] or n_b >= max_symbols[b].
 *   Outputs, all device, caller-owned:
 *     hyps        i32 [minibatch, max_hyp_len]  symbols are appended; nothing else is written (zero-fill it for zero padding)
 *     hyp_lengths i32 [minibatch], scores f32 [minibatch]  written for every hypothesis at every step (f64 sum inside)
 *     emitted     i32 [minibatch]  the symbol hypothesis b emitted in this step, or -1 (blank, done, or paused): the caller
 *                 advances its prediction network for exactly these rows
 *     all_done    i32 [1]  0: some hypothesis is running; 1: every hypothesis is done; 2: none is running, but some are PAUSED
 *                 because they filled max_hyp_len symbols below their max_symbols -- steps with a larger max_hyp_len (a hyps
 *                 buffer grown by the caller, contents kept) resume them
 *     logit_stats f32 [minibatch, 2] or NULL: {max logit, logsumexp} of this step's joint, written for the hypotheses that ran
 *   A hypothesis that is done (or paused) reads nothing and writes only hyp_lengths / scores (unchanged) and emitted = -1.
 *
 * Numerics: the argmax and the max logit are bitwise those of compute_rnnt_joint_logits called with that hypothesis alone
 * (minibatch = maxT = maxU = 1, the same joint_dtype), so a decoder sees the logits the loss was trained on.  The two kernels'
 * call-wide route switches (the direct tanh when some |projection| leaves the e^{2x} table range) are taken per hypothesis, from
 * its own enc_proj row and pred_proj row.  logsumexp: f32 partial sums per 32-symbol chunk, combined in f64.
 * Shapes: joint_dtype 0 (f32-grade) on the shapes compute_rnnt_joint_logits takes for it; joint_dtype 1 (binary16 operands)
 * joint_size a multiple of 128 up to 640 and alphabet_size 1 ... 8192 (padded inside to chunks of 32 symbols that take no part).
 * joint_dtype carries no flag bits.  workspace: get_rnnt_greedy_workspace_size(maxT, minibatch, ...) bytes, 256-byte aligned,
 * owned by one decode from its begin to its last step.  Neither entry point synchronises the host.
 */
RNNT_API rnntStatus_t get_rnnt_greedy_workspace_size(int maxT, int minibatch, int joint_size, int alphabet_size, int joint_dtype,
                                                     size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_greedy_begin(const float *enc_proj, const int *frame_lengths, const int *max_symbols,
                                                const float *W2, const float *b2, int joint_size, int alphabet_size,
                                                int minibatch, int max_per_frame, int joint_dtype, void *workspace,
                                                rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_greedy_step(const float *pred_proj, int *hyps, int max_hyp_len, int *hyp_lengths,
                                               float *scores, int *emitted, int *all_done, float *logit_stats,
                                               int joint_size, int alphabet_size, int minibatch, int joint_dtype,
                                               void *workspace, rnntOptions options);

/* Build-only extension: batched BEAM SEARCH ("modified" beam search: one symbol per frame, frame-synchronous, as the k2 /
 * icefall recipes).  The caller steps the prediction network for every hypothesis row; the library evaluates the joint of
 * every hypothesis (the greedy decoder's: every logit bitwise that of compute_rnnt_joint_logits for the hypothesis alone),
 * ranks the candidates and keeps the beam, without writing logits.
 *
 * Per utterance b (T_b = frame_lengths[b] clamped into [0, maxT]; blank = options.blank_label): the beam holds up to `beam`
 * hypotheses (y, s), y a token sequence, s a float64 log score; at the start [((), 0)].  Per frame t < T_b:
 *   1. per hypothesis i: logits_i = tanh(enc_proj[b, t] + pred_proj[i]) @ W2 + b2 (f32), lse_i = logsumexp(logits_i) (f32
 *      partial sums per 32-symbol chunk, combined in float64, as the greedy decoder forms it);
 *   2. candidates (i, v), score s_i + ((double)logits_i[v] - lse_i) in float64, ranked by score descending, then i, then v
 *      ascending; the first `beam` are taken; NaN and -inf candidates never are; nothing taken: the beam is carried over;
 *   3. a taken candidate's sequence is y_i (v == blank) or y_i + (v,);
 *   4. taken candidates with identical sequences merge: the first-ranked survives with score logaddexp(s_a, s_b) (float64);
 *   5. the new beam is the merged list stably sorted by score, descending (it may hold fewer than `beam` hypotheses).
 * Frames t >= T_b leave the beam as it is.  beam = 1 is greedy decoding with one symbol per frame.
 *
 *   enc_proj      device f32 [minibatch, maxT, joint_size] = enc @ W1 + b1
 *   pred_proj     device f32 [minibatch * beam, joint_size]: row b * beam + k = pred @ W1 of slot k's current prediction output
 *   W2, b2, joint_dtype, shapes: as for the greedy decoder (joint_dtype carries no flag bits); 1 <= beam <= 16
 *   options       loc RNNT_GPU, stream, blank_label (< alphabet_size), maxT (> 0); the same for begin, every step and results
 *
 * compute_rnnt_beam_begin (once per decode) builds the tables and the W2 image and resets every beam to [((), 0)] and its frame
 * counter to 0.  compute_rnnt_beam_step processes the next frame of every utterance:
 *   parents  i32 [minibatch * beam]  the row whose prediction-network state slot r continues (a merged slot: the first-ranked
 *            member's parent -- both have the same sequence); empty and frozen slots: their own row
 *   emitted  i32 [minibatch * beam]  v when slot r's sequence grew by v, else -1: the caller gathers its prediction-network
 *            output and state by `parents`, then advances the rows with emitted >= 0
 *   topk_logits f32 [minibatch * beam, beam], topk_symbols i32 [minibatch * beam, beam], lse f32 [minibatch * beam]: optional
 *            diagnostics (NULL: not written) -- this step's top-`beam` logits of each live hypothesis (logit descending, symbol
 *            ascending; -inf / -1 where there are fewer) and its logsumexp
 * compute_rnnt_beam_results writes the current beams: hyps i32 [minibatch, beam, maxT] (zero-padded), hyp_lengths i32
 * [minibatch, beam], scores f32 [minibatch, beam] (empty slots: length 0, score -inf), best first.
 * workspace: get_rnnt_beam_workspace_size(maxT, minibatch, beam, ...) bytes, 256-byte aligned, owned by one decode from its
 * begin to its results.  No entry point synchronises the host.
 */
RNNT_API rnntStatus_t get_rnnt_beam_workspace_size(int maxT, int minibatch, int beam, int joint_size, int alphabet_size,
                                                   int joint_dtype, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_beam_begin(const float *enc_proj, const int *frame_lengths, const float *W2, const float *b2,
                                              int joint_size, int alphabet_size, int minibatch, int beam, int joint_dtype,
                                              void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_beam_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                             int *topk_symbols, float *lse, int joint_size, int alphabet_size, int minibatch,
                                             int beam, int joint_dtype, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_beam_results(int *hyps, int *hyp_lengths, float *scores, int joint_size, int alphabet_size,
                                                int minibatch, int beam, int joint_dtype, void *workspace, rnntOptions options);

/* Build-only extension: one PREDICTION-NETWORK step for every decoder row (model.py PredictionNetwork, inference only), so that
 * a decode loop is library calls alone: prednet begin, then repeat {greedy / beam step, prednet step}.  The network is an
 * embedding [vocab_size, embed_size] and num_blocks blocks of one single-layer LSTM (torch gate order i, f, g, o; optional
 * bias-free projection) -> LayerNorm (biased variance; dropout is an eval no-op), followed by the joint's first Dense layer
 * without its bias: pred_proj = x @ W1.
 *
 * Per row r = 0 ... rows-1 (rows = minibatch for greedy decoding, minibatch * beam for beam search), with
 * src = parents ? parents[r] : r and tok = emitted[r]:
 *   tok < 0:  row r takes row src's state and pred_proj unchanged (parents == NULL: nothing changes for the row);
 *   tok >= 0: starting from row src's state, x = Emb[tok]; per block l:
 *               gates = W_ih x + b_ih + W_hh r_prev + b_hh;  c = sigma(f) c_prev + sigma(i) tanh(g);  h = sigma(o) tanh(c);
 *               r = W_hr h (projected block) or h;  x = LayerNorm_l(r)
 *             pred_proj[r] = x @ W1.
 * The state of block l is (r [rows, proj], c [rows, hidden]); r is the raw block output before the LayerNorm (torch's h of an
 * LSTM with proj_size).  `emitted` and `parents` are exactly what compute_rnnt_greedy_step / compute_rnnt_beam_step write.
 *
 *   blocks      HOST array of num_blocks rnntPrednetBlock (below); the weight pointers are device f32, 16-byte aligned
 *   embedding   device f32 [vocab_size, embed_size]
 *   W1          device f32 [out, joint_size]: the joint's first Dense layer, zero-padded to joint_size columns (out = the last
 *               block's output width); joint_size a multiple of 64 up to 704 (what the greedy / beam decoders take)
 *   emitted     device i32 [rows]: tokens in [0, vocab_size) or negative (a PRECONDITION: the device does not check tokens)
 *   parents     device i32 [rows] in [0, rows), or NULL
 *   pred_proj_out device f32 [rows, joint_size]: the `pred_proj` of compute_rnnt_greedy_step / compute_rnnt_beam_step
 *   options     loc RNNT_GPU, stream; the other fields are not used
 * Limits: 1 <= rows <= 1024, 1 <= num_blocks <= 8, every width (embed, hidden, proj) in 1 ... 4096; anything else, a NULL
 * pointer or a misaligned one: RNNT_STATUS_INVALID_VALUE, before anything is enqueued.
 *
 * compute_rnnt_prednet_begin (once per decode) packs embedding, every block's weights and W1 into the workspace (the caller may
 * then free or change them), zeroes every row's state and runs the start token 0 (not blank_label) for every row, writing
 * pred_proj_out.  compute_rnnt_prednet_step runs one step as above; the blocks' weight pointers are not read (only the widths
 * and eps must match begin's).  The state and pred_proj are double-buffered in the workspace by step parity, so `parents` may
 * name any row.  Arithmetic: float32, every sum in a fixed order: a row's results are bitwise independent of `rows`, of the
 * other rows and of the run.
 * Workspace: get_rnnt_prednet_workspace_size(...) bytes, 256-byte aligned, owned by one decode from its begin to its last step.
 * It begins with the state: for slot s = (number of begin, step and reset calls so far) & 1, and S = the sum over blocks of
 * A(rows * proj_l) + A(rows * hidden_l) floats, A(n) = n rounded up to a multiple of 64: block l's r [rows, proj_l] sits at float
 * s * S + sum_{m < l} (A(rows proj_m) + A(rows hidden_m)) and its c [rows, hidden_l] right after A(rows proj_l) floats.
 * No entry point synchronises the host.
 */
typedef struct rnntPrednetBlock {
    const float *W_ih;       /* [4 hidden, in]   in = embed_size for block 0, else the previous block's proj */
    const float *W_hh;       /* [4 hidden, proj] */
    const float *b_ih;       /* [4 hidden] */
    const float *b_hh;       /* [4 hidden] */
    const float *W_hr;       /* [proj, hidden], or NULL: no projection (proj must then equal hidden) */
    const float *ln_weight;  /* [proj] LayerNorm gamma */
    const float *ln_bias;    /* [proj] LayerNorm beta */
    int hidden;
    int proj;
    float ln_eps;
} rnntPrednetBlock;

RNNT_API rnntStatus_t get_rnnt_prednet_workspace_size(const rnntPrednetBlock *blocks, int num_blocks, int embed_size,
                                                      int vocab_size, int joint_size, int rows, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_prednet_begin(const float *embedding, const rnntPrednetBlock *blocks, int num_blocks,
                                                 int embed_size, int vocab_size, const float *W1, int joint_size, int rows,
                                                 float *pred_proj_out, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_prednet_step(const int *emitted, const int *parents, float *pred_proj_out,
                                                const rnntPrednetBlock *blocks, int num_blocks, int embed_size, int vocab_size,
                                                int joint_size, int rows, void *workspace, rnntOptions options);

/* Build-only extension: the ENCODER's forward pass for every utterance of a batch (model.py Encoder, inference only), carrying
 * its LSTM state from one run to the next, so that a long input may be encoded in chunks.  The network: a BatchNorm over the
 * feat_size features with running statistics, x' = (x - bn_mean) * bn_weight / sqrt(bn_var + bn_eps) + bn_bias, then
 * num_layers blocks of one single-layer LSTM (torch gate order i, f, g, o; optional bias-free projection) -> LayerNorm (biased
 * variance; dropout is an eval no-op), described by the rnntPrednetBlock struct above (block 0's in = feat_size).  After block
 * reduction_index, TimeReduction stacks reduction_factor = f consecutive frames of the LayerNorm output into one row of f times
 * the width (block reduction_index + 1's in = f * proj); a frame past the end of the run's input reads as ZEROS (the pad comes
 * after the LayerNorm).  Padded frames are run through, as in the reference.
 *
 * Per row r = 0 ... rows-1 (one utterance each) and block l with state (r_l [rows, proj_l], c_l [rows, hidden_l]):
 *   for every frame t of the block's input:  gates = W_ih x_t + b_ih + W_hh r + b_hh;  c = sigma(f) c + sigma(i) tanh(g);
 *                                            h = sigma(o) tanh(c);  r = W_hr h (projected block) or h
 * r is the raw block output before the LayerNorm (torch's h of an LSTM with proj_size).
 *
 *   blocks       HOST array of num_layers rnntPrednetBlock; the weight pointers are device f32, 16-byte aligned
 *   bn_*         device f32 [feat_size]
 *   x            device f32 [rows, frames, feat_size], contiguous
 *   out          device f32 [rows, ceil(frames / f), out_width]: the last block's LayerNorm output (out_width = its proj)
 *   options      loc RNNT_GPU, stream; the other fields are not used
 * Limits: 1 <= rows <= 1024, 1 <= num_layers <= 16, every width (feat, hidden, proj, f * proj at the reduction) in 1 ... 4096,
 * 0 <= reduction_index < num_layers - 1, 1 <= reduction_factor <= 16, 1 <= frames <= max_frames <= 2^20; anything else, a NULL
 * pointer or a misaligned one: RNNT_STATUS_INVALID_VALUE, before anything is enqueued.
 *
 * compute_rnnt_encoder_begin packs every block's weights and the BatchNorm into the workspace (the caller may then free or change
 * them) and zeroes every row's state.  compute_rnnt_encoder_run encodes `frames` more frames of every row and advances the state;
 * the blocks' weight pointers are not read (only the widths and eps must match begin's).
 * Chunking: each run pads its own odd tail at the reduction, as TimeReduction does per call.  Runs whose lengths are multiples of
 * f, except the last, give bit-identical output and state to one run over the concatenation.
 * Arithmetic: float32, every sum in a fixed order: a row's results are bitwise independent of `rows`, of the other rows and of
 * the run.
 * Workspace: get_rnnt_encoder_workspace_size(...) bytes, 256-byte aligned, owned by one stream from begin to its last run.  It
 * begins with the state: with A(n) = n rounded up to a multiple of 64, block l's r [rows, proj_l] sits at float
 * sum_{m < l} (A(rows proj_m) + A(rows hidden_m)) and its c [rows, hidden_l] right after A(rows proj_l) floats.
 * No entry point synchronises the host.
 */
RNNT_API rnntStatus_t get_rnnt_encoder_workspace_size(const rnntPrednetBlock *blocks, int num_layers, int feat_size,
                                                      int reduction_index, int reduction_factor, int rows, int max_frames,
                                                      size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_encoder_begin(const rnntPrednetBlock *blocks, int num_layers, int feat_size,
                                                 const float *bn_mean, const float *bn_var, const float *bn_weight,
                                                 const float *bn_bias, float bn_eps, int reduction_index, int reduction_factor,
                                                 int rows, int max_frames, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_encoder_run(const float *x, int frames, float *out, const rnntPrednetBlock *blocks,
                                               int num_layers, int feat_size, float bn_eps, int reduction_index,
                                               int reduction_factor, int rows, int max_frames, void *workspace,
                                               rnntOptions options);

/* The same over RAGGED rows with a per-row reset, for streams that start and end at different times.  Before the run, the rows
 * with reset[r] != 0 start from zero state (reset NULL: none).  Row r then advances over its first row_frames[r] frames only
 * (device i32 [rows], clamped into [0, frames]); a row with 0 frames keeps its state bit for bit.  At the reduction, a frame at or
 * beyond row_frames[r] reads as ZEROS, and `out` is zero past the row's ceil(row_frames[r] / f) frames.  The saved state is that
 * of the row's last valid frame.  The input GEMM may still compute the dead frames; nothing of them is kept.  With equal
 * row_frames = frames and no reset this is compute_rnnt_encoder_run bit for bit; a row run alone gives bitwise the same output
 * and state. */
RNNT_API rnntStatus_t compute_rnnt_encoder_run_rows(const float *x, int frames, const int *row_frames, const int *reset, float *out,
                                                    const rnntPrednetBlock *blocks, int num_layers, int feat_size, float bn_eps,
                                                    int reduction_index, int reduction_factor, int rows, int max_frames,
                                                    void *workspace, rnntOptions options);

/* Build-only extension: STREAMING GREEDY DECODING over S slots (1 <= S <= 1024), each holding one live stream at a time.  The
 * caller feeds every slot zero or more new spectrogram frames per call; the encoder (compute_rnnt_encoder_run_rows), the
 * prediction network and the greedy search carry their state from one feed to the next.
 *
 * compute_rnnt_prednet_reset: one prediction-network step in which the rows with reset[r] != 0 (device i32 [rows]) get zero
 * state and run the start token 0 -- bitwise what compute_rnnt_prednet_begin computes for them -- while the other rows keep
 * their state and pred_proj.  It counts as a step for the parity slot of the workspace layout above (slot = the number of
 * begin, step and reset calls so far, & 1), so the next compute_rnnt_prednet_step reads the right slot.
 *
 * The greedy stream: options.maxT = max_chunk_frames (the encoder frames one feed may bring per slot), minibatch = slots.
 *   get_rnnt_greedy_stream_workspace_size(max_chunk_frames, slots, enc_width, ...): the greedy workspace of
 *     get_rnnt_greedy_workspace_size(max_chunk_frames, slots, ...) followed by W1 [enc_width, joint_size] and b1 [joint_size];
 *     compute_rnnt_greedy_step runs on it unchanged (with the same options and minibatch = slots).
 *   compute_rnnt_greedy_stream_begin(W1, b1, W2, b2, ...) packs W1, b1 and the W2 image (the caller may then free them) and
 *     leaves every slot FINISHED.
 *   compute_rnnt_greedy_stream_feed(enc, enc_frames, chunk_frames, reset, final_chunk, max_symbols, max_per_frame, hyp_lengths,
 *     scores, all_done, ...):
 *       enc           device f32 [slots, enc_frames, enc_width] (0 <= enc_frames <= max_chunk_frames; NULL when 0): this feed's
 *                     encoder frames; slot s uses its first chunk_frames[s] (device i32, clamped into [0, enc_frames])
 *       reset         device i32 [slots] or NULL: reset[s] != 0 starts a new stream in slot s: no symbols, score 0, budget
 *                     max_symbols[s] (NULL: none beyond the hyps buffer), per-frame cap max_per_frame (<= 0: none)
 *       final_chunk   device i32 [slots] or NULL: final_chunk[s] != 0: the stream in slot s ends with this chunk
 *     It projects the chunk's frames through W1 + b1 (one f32 FMA chain per output over enc_width in order, then + b1: a frame's
 *     enc_proj is bitwise independent of the chunking, the slot and S), builds the e^{2x} tables and range flags of those frames,
 *     and moves every slot on: a live slot gets frame cursor 0 over chunk_frames[s] frames and keeps its symbols, score and
 *     budget; a finished slot (after its final chunk, or once its budget is spent) stays done until a reset.  It writes
 *     hyp_lengths / scores of every slot and all_done (0: some slot has frames to decode, 1: none).
 *   Then repeat {compute_rnnt_greedy_step, compute_rnnt_prednet_step} until all_done is 1 (2: grow `hyps` as for the batched
 *   decoder).  `hyps` [slots, max_hyp_len] is the per-stream, append-only buffer of the batched decoder: symbol n of the stream
 *   in slot s sits at hyps[s, n].  A slot that has used up its chunk is done for the step loop; the next feed brings it back.
 * Equivalence: a stream fed through chunks whose lengths are multiples of the encoder's reduction factor (the last one
 * excepted), in any slot, beside any other traffic, gives bitwise the ids, length and score of the same stream fed in one call
 * to a 1-slot decoder.  No entry point synchronises the host; bad arguments give RNNT_STATUS_INVALID_VALUE before anything is
 * enqueued. */
RNNT_API rnntStatus_t compute_rnnt_prednet_reset(const int *reset, float *pred_proj_out, const rnntPrednetBlock *blocks,
                                                 int num_blocks, int embed_size, int vocab_size, int joint_size, int rows,
                                                 void *workspace, rnntOptions options);

RNNT_API rnntStatus_t get_rnnt_greedy_stream_workspace_size(int max_chunk_frames, int slots, int enc_width, int joint_size,
                                                            int alphabet_size, int joint_dtype, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_greedy_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2,
                                                       int enc_width, int joint_size, int alphabet_size, int slots,
                                                       int joint_dtype, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_greedy_stream_feed(const float *enc, int enc_frames, const int *chunk_frames, const int *reset,
                                                      const int *final_chunk, const int *max_symbols, int max_per_frame,
                                                      int *hyp_lengths, float *scores, int *all_done, int enc_width,
                                                      int joint_size, int alphabet_size, int slots, int joint_dtype,
                                                      void *workspace, rnntOptions options);

/* Build-only extension: STREAMING BEAM SEARCH over S slots: the beam search of compute_rnnt_beam_* fed chunk by chunk as the
 * greedy stream is, each slot keeping its beam from one feed to the next.  S = slots, K = beam, N = max_hyp_len (the tokens one
 * stream's hypothesis may hold); options.maxT = max_chunk_frames.  Limits: 1 <= K <= 16, 1 <= S, S K <= 1024 (the prediction
 * network's rows), 1 <= N, 2 S K N < 2^31, 1 <= enc_width <= 4096; joint_size, alphabet_size, joint_dtype (no flag bits) and
 * options (loc RNNT_GPU, stream, blank_label < alphabet_size, maxT > 0; the same for every call) as for the beam decoder.
 *
 *   get_rnnt_beam_stream_workspace_size(max_chunk_frames, slots, beam, max_hyp_len, enc_width, ...): the beam workspace for
 *     (max_chunk_frames, S, K) with token rows of stride N instead of maxT, followed by W1 [enc_width, joint_size] and
 *     b1 [joint_size].  256-byte aligned; it grows with N and K; it holds 2 S K N token words.
 *   compute_rnnt_beam_stream_begin(W1, b1, W2, b2, ...) packs W1, b1 and the W2 image (the caller may then free them) and leaves
 *     every slot FINISHED with an EMPTY beam (no hypothesis at all).
 *   compute_rnnt_beam_stream_feed(enc, enc_frames, chunk_frames, reset, final_chunk, ...): enc, enc_frames, chunk_frames, reset
 *     and final_chunk exactly as for compute_rnnt_greedy_stream_feed.  It projects the chunk's frames through W1 + b1 with the
 *     greedy stream's projection (one f32 FMA chain per output: a frame's enc_proj is bitwise independent of the chunking, the
 *     slot and S), builds the e^{2x} tables and range flags of those frames, and moves every slot on:
 *       reset[s] != 0      the beam becomes [((), 0)], the slot's step count 0, and the slot is not finished;
 *       a live slot        gets frame cursor 0 over chunk_frames[s] frames and keeps its beam and step count;
 *       a finished slot    stays frozen (its beam readable) until a reset;
 *       final_chunk[s]     != 0 finishes the slot after this chunk's frames.
 *   compute_rnnt_beam_stream_step(pred_proj, parents, emitted, topk_logits, topk_symbols, lse, ...): one frame of every slot that
 *     has one left in its chunk, by rules 1 - 5 of compute_rnnt_beam_step (minibatch = slots), with the same outputs; slots
 *     without a frame left are frozen: parents = own row, emitted = -1.  One rule is added: a hypothesis that already holds N
 *     tokens offers only its blank candidate (i, blank), whatever rank blank has among its logits; its other candidates are never
 *     taken, exactly like -inf candidates (topk_logits / topk_symbols still show its plain top-`beam`).  The rule cannot fire in
 *     compute_rnnt_beam_step, where a hypothesis holds at most one token per frame of maxT.
 *   compute_rnnt_beam_stream_results(hyps, hyp_lengths, scores, stable_lengths, ...): the current beams, best first: hyps i32
 *     [S, K, N] zero-padded, hyp_lengths i32 [S, K], scores f32 [S, K]; stable_lengths i32 [S] or NULL: the length of the longest
 *     common prefix of all occupied hypotheses of slot s -- the tokens no later frame can change (every later hypothesis extends
 *     one of these).  It never exceeds the shortest occupied hypothesis.  An empty or never-started slot: lengths 0, scores
 *     -inf, stable_lengths 0.  Callable between any two calls of the stream; it changes nothing.
 *
 * The loop, per chunk: feed; then max over s of chunk_frames[s] times {compute_rnnt_beam_stream_step;
 * compute_rnnt_prednet_step(emitted, parents)}.  The number of steps is host data: nothing is polled.  The prediction network is
 * stepped after the LAST frame of a feed too (the offline loop may skip that step; the stream must not), so that the next chunk
 * starts from the state of the hypotheses it continues.  A new stream in slot s resets its K prediction-network rows
 * s K ... s K + K-1 with compute_rnnt_prednet_reset and its encoder row with compute_rnnt_encoder_run_rows' reset.
 * Equivalence: a stream fed through chunks whose lengths are multiples of the encoder's reduction factor (the last one excepted),
 * in any slot, beside any other traffic, gives bitwise the n-best (ids, lengths, f32 scores) and stable_lengths of the same
 * stream fed in one call to a 1-slot decoder.  Cost: the select kernel copies every surviving token row each frame, O(length).
 * No entry point synchronises the host; the caller owns every buffer; a NULL (where not allowed above) or misaligned pointer
 * (workspace: 256 bytes; every other: 4), a shape outside the limits, enc_frames > max_chunk_frames or options.loc != RNNT_GPU
 * give RNNT_STATUS_INVALID_VALUE before anything is enqueued. */
RNNT_API rnntStatus_t get_rnnt_beam_stream_workspace_size(int max_chunk_frames, int slots, int beam, int max_hyp_len, int enc_width,
                                                          int joint_size, int alphabet_size, int joint_dtype, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_beam_stream_begin(const float *W1, const float *b1, const float *W2, const float *b2,
                                                     int enc_width, int joint_size, int alphabet_size, int slots, int beam,
                                                     int max_hyp_len, int joint_dtype, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_beam_stream_feed(const float *enc, int enc_frames, const int *chunk_frames, const int *reset,
                                                    const int *final_chunk, int enc_width, int joint_size, int alphabet_size,
                                                    int slots, int beam, int max_hyp_len, int joint_dtype, void *workspace,
                                                    rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_beam_stream_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                                    int *topk_symbols, float *lse, int joint_size, int alphabet_size, int slots,
                                                    int beam, int max_hyp_len, int joint_dtype, void *workspace,
                                                    rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_beam_stream_results(int *hyps, int *hyp_lengths, float *scores, int *stable_lengths,
                                                       int joint_size, int alphabet_size, int slots, int beam, int max_hyp_len,
                                                       int joint_dtype, void *workspace, rnntOptions options);

/* Build-only extension: PER-TOKEN EMISSION FRAMES AND LOG-PROBABILITIES from the four decoders above ("timed" decoding).  New
 * entry points only: every function above keeps its signature, its results bit for bit and what its size query returns; the
 * timed calls compute ids, lengths and scores bitwise equal to the untimed ones.  joint_dtype carries no flag bits here either.
 *
 * Definitions.
 *   emission frame of a token  the 0-based encoder frame t whose joint evaluation made the decision that appended the token
 *                    (token_frames of compute_rnnt_align has the same convention).  Offline t counts from the utterance's first
 *                    frame; on a stream it counts from the slot's reset, across every chunk fed since.
 *   log-probability of a token (double)logit[v] - lse of that decision -- the float64 term the decision added to the hypothesis
 *                    score -- rounded once to f32.
 *   beam merges      when rule 4 of compute_rnnt_beam_step merges taken candidates with identical token sequences, the
 *                    first-ranked survivor keeps ITS OWN frames and log-probabilities; the merged score stays the logaddexp of
 *                    the members.  Frames and log-probabilities describe one path; the score may sum several.
 *   timed stable length (beam stream)  the length of the longest prefix on which all occupied hypotheses of a slot agree in
 *                    token AND in emission frame.  Every later hypothesis descends from one of the current ones and a merge
 *                    keeps one member's rows, so nothing in this prefix, times included, can change any more.  It never exceeds
 *                    stable_lengths, which compares tokens only.
 *
 * Greedy, batched and streaming (they share the step):
 *   compute_rnnt_greedy_step_timed is compute_rnnt_greedy_step plus hyp_frames i32 [minibatch, max_hyp_len] and hyp_logp f32
 *     [minibatch, max_hyp_len], caller-owned, append-only, written at the position of hyps[b, n_b] and nowhere else.  A caller that
 *     grows hyps after all_done == 2 grows and copies all three buffers.  frame_base i32 [minibatch] or NULL (0): added to the
 *     frame of every token of row b; the batched decoder passes NULL.  Timed and untimed steps may be mixed on one workspace.
 *   compute_rnnt_greedy_stream_feed_timed is compute_rnnt_greedy_stream_feed plus frame_base i32 [slots], caller-owned state the
 *     feed keeps: a reset sets frame_base[s] = 0, every other feed adds the frames of the chunk the slot had before this one.
 *     Passed to compute_rnnt_greedy_step_timed, it makes the frames absolute since the slot's reset.  Its content means nothing
 *     before a slot's first reset (the slot emits nothing then).  The workspace is that of
 *     get_rnnt_greedy_stream_workspace_size, unchanged; a stream uses the timed feed for all its feeds or for none.
 * Beam, batched: get_rnnt_beam_timed_workspace_size, compute_rnnt_beam_timed_begin / _step / _results are the untimed four on a
 *   workspace that holds, beside the double-buffered token rows, a double-buffered row of {frame, log-probability} pairs (8
 *   bytes per token) per hypothesis, gathered by parent exactly as the tokens.  _results adds hyp_frames i32 [minibatch, beam,
 *   maxT] (padded with -1) and hyp_logp f32 [minibatch, beam, maxT] (padded with 0), as compute_rnnt_align pads them.
 * Beam, streaming: get_rnnt_beam_stream_timed_workspace_size, compute_rnnt_beam_stream_timed_begin / _feed / _step / _results
 *   likewise ([slots, beam, max_hyp_len]); _results also writes timed_stable_lengths i32 [slots] (NULL: not written).
 *   A workspace is used by the timed calls or by the untimed ones, never both.
 * Limits: the untimed beam workspace holds 2 S K N token words (2 S K N < 2^31); the timed one adds 4 S K N words, and
 *   6 S K N < 2^31 is required (S = minibatch or slots, K = beam, N = maxT or max_hyp_len).
 * Equivalence: the guarantee of the streams extends to hyp_frames, hyp_logp and timed_stable_lengths, bitwise.
 * Validation as everywhere: a NULL (where not allowed) or misaligned pointer (workspace: 256 bytes; every other: 4), a shape
 * outside the limits or flag bits in joint_dtype give RNNT_STATUS_INVALID_VALUE before anything is enqueued.  No entry point
 * synchronises the host. */
RNNT_API rnntStatus_t compute_rnnt_greedy_step_timed(const float *pred_proj, int *hyps, int *hyp_frames, float *hyp_logp,
                                                     int max_hyp_len, int *hyp_lengths, float *scores, int *emitted, int *all_done,
                                                     float *logit_stats, const int *frame_base, int joint_size, int alphabet_size,
                                                     int minibatch, int joint_dtype, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_greedy_stream_feed_timed(const float *enc, int enc_frames, const int *chunk_frames,
                                                            const int *reset, const int *final_chunk, const int *max_symbols,
                                                            int max_per_frame, int *hyp_lengths, float *scores, int *all_done,
                                                            int *frame_base, int enc_width, int joint_size, int alphabet_size,
                                                            int slots, int joint_dtype, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t get_rnnt_beam_timed_workspace_size(int maxT, int minibatch, int beam, int joint_size, int alphabet_size,
                                                         int joint_dtype, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_beam_timed_begin(const float *enc_proj, const int *frame_lengths, const float *W2,
                                                    const float *b2, int joint_size, int alphabet_size, int minibatch, int beam,
                                                    int joint_dtype, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_beam_timed_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                                   int *topk_symbols, float *lse, int joint_size, int alphabet_size, int minibatch,
                                                   int beam, int joint_dtype, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_beam_timed_results(int *hyps, int *hyp_lengths, float *scores, int *hyp_frames, float *hyp_logp,
                                                      int joint_size, int alphabet_size, int minibatch, int beam, int joint_dtype,
                                                      void *workspace, rnntOptions options);

RNNT_API rnntStatus_t get_rnnt_beam_stream_timed_workspace_size(int max_chunk_frames, int slots, int beam, int max_hyp_len,
                                                                int enc_width, int joint_size, int alphabet_size, int joint_dtype,
                                                                size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_beam_stream_timed_begin(const float *W1, const float *b1, const float *W2, const float *b2,
                                                           int enc_width, int joint_size, int alphabet_size, int slots, int beam,
                                                           int max_hyp_len, int joint_dtype, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_beam_stream_timed_feed(const float *enc, int enc_frames, const int *chunk_frames,
                                                          const int *reset, const int *final_chunk, int enc_width, int joint_size,
                                                          int alphabet_size, int slots, int beam, int max_hyp_len, int joint_dtype,
                                                          void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_beam_stream_timed_step(const float *pred_proj, int *parents, int *emitted, float *topk_logits,
                                                          int *topk_symbols, float *lse, int joint_size, int alphabet_size,
                                                          int slots, int beam, int max_hyp_len, int joint_dtype, void *workspace,
                                                          rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_beam_stream_timed_results(int *hyps, int *hyp_lengths, float *scores, int *stable_lengths,
                                                             int *hyp_frames, float *hyp_logp, int *timed_stable_lengths,
                                                             int joint_size, int alphabet_size, int slots, int beam,
                                                             int max_hyp_len, int joint_dtype, void *workspace,
                                                             rnntOptions options);

/* Build-only extension: ONE LSTM LAYER FOR TRAINING -- a forward pass that keeps what the backward needs, and back-propagation
 * through time.  rows R (the batch), frames T, hidden H, output width P: a projected layer (W_hr [P, H] given, P < H, bias-free)
 * or an unprojected one (W_hr NULL, P = H).  torch's gate order i, f, g, o; zero initial state; no row lengths (padded frames
 * are run through like any other).  Every buffer is device f32, 16-byte aligned and TIME-MAJOR: a frame's R rows are contiguous.
 *
 *   forward, t = 0 ... T-1:   a_t = pre_t + r_{t-1} W_hh^T;  i, f, o = sigma(a_i), sigma(a_f), sigma(a_o);  g = tanh(a_g);
 *                             c_t = f c_{t-1} + i g;  h_t = o tanh(c_t);  r_t = h_t W_hr^T (projected) or h_t
 *   backward, t = T-1 ... 0:  dr_t = dy_t + da_{t+1} W_hh;  dh_t = dr_t W_hr (projected) or dr_t;
 *                             dc_t = dh_t o (1 - tanh^2 c_t) + dc_{t+1} f_{t+1};
 *                             da_i = dc_t g i (1 - i);  da_f = dc_t c_{t-1} f (1 - f);  da_g = dc_t i (1 - g^2);
 *                             da_o = dh_t tanh(c_t) o (1 - o)
 *
 * compute_rnnt_lstm_train_fwd(gates, W_hh, W_hr, y, c, h, ...):
 *   gates  [T, R, 4H]  in: pre = x W_ih^T + b_ih + b_hh of every frame (the caller's GEMM), columns i | f | g | o as torch
 *                      stores them; OVERWRITTEN by the activated gates i, f, g, o
 *   W_hh   [4H, P], W_hr [P, H] or NULL: as torch stores them; packed into the workspace on every call (weights change every step)
 *   y      [T, R, P]   out: r_t, the layer's output       c  [T, R, H]  out: every c_t
 *   h      [T, R, H]   out, projected layers only (NULL otherwise): every h_t
 * compute_rnnt_lstm_train_bwd(gates, c, dy, W_hh, W_hr, dr, ...):
 *   gates  [T, R, 4H]  in: the forward's activated gates; OVERWRITTEN by da (same columns)
 *   c      [T, R, H]   the forward's c                     dy [T, R, P]  the gradient of y
 *   dr     [T, R, P]   out, projected layers only (NULL otherwise): every dr_t
 * Everything that is not recurrent is then a sum over all frames at once and is left to the caller's GEMMs:
 *   dW_ih = da^T x;  dW_hh = da[1:]^T y[:-1];  db_ih = db_hh = sum da;  dx = da W_ih;  dW_hr = dr^T h.
 *
 * Launches: one per frame for an unprojected layer and two for a projected one, in each direction, plus one pack per matrix and
 * call.  No kernel waits for another workgroup; the frame-to-frame dependency is stream order.
 * Arithmetic: float32, every sum in an order fixed by the shapes alone: a row's y, c, h, gates, da and dr are bitwise
 * independent of `rows`, of the other rows and of the call.  Against a float64 LSTM the forward stays within
 * 1e-4 max(1, max|ref|).
 * Limits: 1 <= rows <= 1024, 1 <= frames <= 2^20, 1 <= proj <= hidden <= 4096, proj < hidden exactly when W_hr is given; anything
 * else, a NULL or misaligned pointer, or options.loc != RNNT_GPU: RNNT_STATUS_INVALID_VALUE, before anything is enqueued.
 * Workspace: get_rnnt_lstm_train_workspace_size(rows, frames, hidden, proj) bytes (a projected layer when proj < hidden),
 * 256-byte aligned, owned by the call's stream for the call: the weight images and the backward's dc carry.  Nothing is kept in
 * it between the forward and the backward.  No entry point synchronises the host. */
RNNT_API rnntStatus_t get_rnnt_lstm_train_workspace_size(int rows, int frames, int hidden, int proj, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_lstm_train_fwd(float *gates, const float *W_hh, const float *W_hr, float *y, float *c, float *h,
                                                  int rows, int frames, int hidden, int proj, void *workspace,
                                                  rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_lstm_train_bwd(float *gates, const float *c, const float *dy, const float *W_hh,
                                                  const float *W_hr, float *dr, int rows, int frames, int hidden, int proj,
                                                  void *workspace, rnntOptions options);

/* Build-only extension: the STREAMING LOG-MEL FRONT END over S slots (1 <= S <= 1024): raw audio chunks in, stacked log-mel rows
 * out -- what compute_rnnt_encoder_run_rows and the streaming decoders take -- with the state of every stream kept in the
 * workspace.  The spectral definitions are those of tf.signal.stft / linear_to_mel_weight_matrix as the offline front end
 * restates them: L = frame_len samples per frame, frame_step <= L samples between frames, nfft = the next power of two >= L
 * (256, 512, 1024 or 2048), magnitude of the one-sided spectrum, mel = |X| @ mel_weights summed per filter over its band (first
 * to last non-zero weight) in ascending bin order, x = log(mel + 1e-6) (the sum in float32; the log in float64, rounded once).
 * stack = the frames side by side in one row (downsample_spec), row_multiple = the encoder's reduction factor, G = stack *
 * row_multiple, M = mel_bins.
 *
 * State per slot: c < L carried samples, n frames made so far, the running per-bin sum m [M], h < G held frames, a finished flag.
 * Feed of k new samples (0 <= k <= chunk_samples <= max_chunk_samples; samples[s] is clamped into that range) to a live slot:
 *   avail = c + k;  nf = avail < L ? 0 : 1 + (avail - L) / frame_step;  c' = avail - nf frame_step
 *   (frame i of a stream always covers its samples i frame_step ... i frame_step + L - 1)
 *   each new frame, in stream order:  norm 0: y = x;   norm 1: n += 1; m += x; y = x - (m / n + 1e-8)   (float32, per bin)
 *   not final:  (h + nf) / G * row_multiple rows leave, (h + nf) % G frames are held
 *   final:      (h + nf) / stack rows leave; the other frames and the carried samples are dropped; the slot is FINISHED
 * A finished slot ignores feeds (0 rows, nothing changes) until reset[s] != 0, which zeroes its state and makes it live BEFORE the
 * call's samples are taken.  Row r of a slot is its frames r stack ... r stack + stack-1 side by side, [M * stack].
 *
 *   max_rows = (G - 1 + NF) / stack with NF = 1 + (max_chunk_samples - 1) / frame_step: a feed completes at most NF frames
 *   (avail <= L - 1 + max_chunk_samples) beside at most G - 1 held ones.  row_counts are a function of the sample counts alone:
 *   a caller mirrors them in integers and need never read them back.
 *
 *   window        device f32 [frame_len] (the periodic Hann window; formed in float64, rounded once)
 *   mel_weights   device f32 [nfft / 2 + 1, mel_bins] (formed in float64, rounded once)
 *   audio         device f32 [slots, chunk_samples], contiguous (NULL when chunk_samples is 0)
 *   samples       device i32 [slots];  reset, final_chunk: device i32 [slots] or NULL (none)
 *   rows_out      device f32 [slots, max_rows, mel_bins * stack]: rows past a slot's count are written as ZEROS
 *   row_counts    device i32 [slots]
 *   options       loc RNNT_GPU, stream; the other fields are not used
 * compute_rnnt_frontend_begin copies the window, packs the mel matrix (transposed, with every filter's band) and the FFT's
 * twiddles (float64, rounded once) into the workspace -- the caller may then free them -- and leaves every slot FINISHED.
 * compute_rnnt_frontend_feed is two launches: the new frames of every slot (one wave per frame: gather, window, FFT in LDS,
 * magnitude, band sum, log), then per slot the scan in stream order, the rows, the held frames and the new carry, which is
 * written only there, after every frame has been read.
 * Equivalence: every sum has an order fixed by the shapes alone, so a frame is bitwise independent of the chunking, the slot, S
 * and the other slots' traffic: a stream fed through any chunks (zero-sample feeds and chunks shorter than a step included) gives
 * bitwise the rows, in the same total number, of the same stream fed in one call to a 1-slot front end.
 * Limits: 1 <= max_chunk_samples <= 2^20, 1 <= frame_step <= frame_len, 129 <= frame_len <= 2048, 1 <= mel_bins <= 1024,
 * 1 <= stack, row_multiple <= 16, norm 0 or 1; anything else, chunk_samples outside 0 ... max_chunk_samples, a NULL (where not
 * allowed above) or misaligned pointer (workspace: 256 bytes; every other: 4) or options.loc != RNNT_GPU:
 * RNNT_STATUS_INVALID_VALUE, before anything is enqueued.  Workspace: get_rnnt_frontend_workspace_size(...) bytes, owned by the
 * S streams from begin on.  No entry point synchronises the host. */
RNNT_API rnntStatus_t get_rnnt_frontend_workspace_size(int max_chunk_samples, int slots, int frame_len, int frame_step,
                                                       int mel_bins, int stack, int row_multiple, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_frontend_begin(const float *window, const float *mel_weights, int max_chunk_samples, int slots,
                                                  int frame_len, int frame_step, int mel_bins, int stack, int row_multiple,
                                                  void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_frontend_feed(const float *audio, int chunk_samples, const int *samples, const int *reset,
                                                 const int *final_chunk, int norm, float *rows_out, int *row_counts,
                                                 int max_chunk_samples, int slots, int frame_len, int frame_step, int mel_bins,
                                                 int stack, int row_multiple, void *workspace, rnntOptions options);

/* ------------------------------------------------------------------------------------------
 * Build-only extension (no upstream counterpart): FORCED ALIGNMENT -- the maximum-probability monotone path through the
 * T x (U+1) lattice the loss sums over, and the frame at which it emits every label.
 *
 * Convention of compute_rnnt_loss: acts f32 [minibatch, maxT, maxU, alphabet_size] RAW LOGITS, maxU = longest label sequence + 1,
 * T_b = input_lengths[b], U_b = label_lengths[b], flat_labels [minibatch, maxU-1], blank = options.blank_label.  Per utterance:
 *   lpb[t,u] = log_softmax(acts[b,t,u,:])[blank]
 *   lpl[t,u] = log_softmax(acts[b,t,u,:])[label_b[u]]            u < U_b
 *   v(0,0)   = 0
 *   v(t,u)   = max( v(t-1,u) + lpb[t-1,u] , v(t,u-1) + lpl[t,u-1] )
 *   score_b  = v(T_b-1, U_b) + lpb[T_b-1, U_b]
 * Tie rule (part of the contract): a cell with two predecessors takes the label arrival, from (t, u-1), only if its value is
 * STRICTLY greater; on an exact tie it takes the blank arrival, from (t-1, u).  A cell with one predecessor takes that one.
 * Outputs, from the back-trace that starts at (T_b-1, U_b):
 *   token_frames  device i32 [minibatch, maxU-1]  the frame t at which label u is emitted on the best path; -1 for u >= U_b.
 *                                                 Non-decreasing in u; several labels may share a frame.
 *   token_logp    device f32 [minibatch, maxU-1]  lpl[token_frames[b,u], u], the per-token confidence; 0 for u >= U_b
 *   scores        device f32 [minibatch]          the best path's log-probability (natural log)
 * U_b = 0 is valid: the path is all blanks, every token_frames entry is -1.  Out-of-range lengths (T_b < 1, T_b > maxT, U_b < 0,
 * U_b > maxU-1) are device data, as in the op: they are clamped into the tensor and THAT utterance comes back with a NaN score,
 * -1 frames and 0 confidences; nothing else in the batch is affected.  Labels outside [0, alphabet_size) are clamped into range.
 * Arithmetic: the normaliser of every cell in float32 from the float32 logits (running max / sum of exponentials); the sweep
 * carries v in float64, so the T_b + U_b additions along a path add no error of their own.  Every sum has an order fixed by the
 * shapes alone (the normaliser's by alphabet_size, the sweep's by the utterance's own cells): an utterance's three outputs are
 * BITWISE independent of the rest of the batch, of minibatch and of how the frames were cut into slabs.  Cells outside an
 * utterance's T_b x (U_b+1) lattice are neither read from acts nor from the workspace.
 *
 *   get_rnnt_align_workspace_size  bytes for (maxT, maxU, minibatch): two f32 per lattice cell on a row stride of maxU rounded up
 *                                  to the sweep's width (64 x columns per lane; 1024 x columns per thread above 1024 columns), one
 *                                  decision BIT per cell.  Never depends on alphabet_size.
 *   compute_rnnt_align_cells       acts_slab f32 [minibatch, slab_frames, maxU, alphabet_size] = the logits of frames
 *                                  frame_offset ... frame_offset + slab_frames - 1 of every utterance: writes their lpb / lpl
 *                                  into the workspace.  A caller that produces logits slab by slab (alphabet_size 4096) never
 *                                  holds [B, T, U, V]: it reduces each slab to two floats per cell and reuses the slab buffer.
 *   compute_rnnt_align_path        the sweep and the back-trace on what a sequence of _cells calls covering frames 0 ... maxT-1
 *                                  (in any order, any slab sizes) has left in the workspace.
 *   compute_rnnt_align             = _cells on the whole tensor (slab_frames = maxT, frame_offset 0) followed by _path.
 * Domain: the op's -- maxU <= 8192, minibatch * maxT * maxU < 2^31, any alphabet_size >= 2, 0 <= blank_label < alphabet_size,
 * options.loc == RNNT_GPU, batch_first; 1 <= slab_frames, 0 <= frame_offset, frame_offset + slab_frames <= maxT.  Pointers:
 * none may be NULL; workspace 256-byte aligned, every other 4-byte aligned (acts_slab 16-byte aligned with alphabet_size a
 * multiple of 4 takes the wide loads; results do not depend on it).  Anything else: RNNT_STATUS_INVALID_VALUE before anything is
 * enqueued.  No entry point synchronises the host. */
RNNT_API rnntStatus_t get_rnnt_align_workspace_size(int maxT, int maxU, int minibatch, size_t *size_bytes);

RNNT_API rnntStatus_t compute_rnnt_align_cells(const float *acts_slab, int slab_frames, int frame_offset, const int *flat_labels,
                                               const int *label_lengths, const int *input_lengths, int alphabet_size,
                                               int minibatch, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_align_path(int *token_frames, float *token_logp, float *scores, const int *label_lengths,
                                              const int *input_lengths, int minibatch, void *workspace, rnntOptions options);

RNNT_API rnntStatus_t compute_rnnt_align(const float *acts, const int *flat_labels, const int *label_lengths,
                                         const int *input_lengths, int alphabet_size, int minibatch, int *token_frames,
                                         float *token_logp, float *scores, void *workspace, rnntOptions options);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_RNNT_H */
