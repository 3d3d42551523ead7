// rnnt_joint_math.h -- h = tanh(enc_proj + pred_proj) as every joint kernel forms it (joint_kernels.hip, joint_f16_kernels.hip,
// greedy_kernels.hip).  One definition, so that the decoder's step kernel rounds exactly as the loss's forward kernels do.
#pragma once
#include "rnnt_common.h"

namespace rnnt {

// tanh(x) = 1 - 2/(1+e^{2x}); saturates correctly at +-inf, absolute error ~1e-7
__device__ __forceinline__ float fast_tanh(float x) {
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * 2.8853900817779268f));
}
// tanh(a + c) from the tabulated factors ea = e^{2a}, ec = e^{2c} (exp_tab): one multiply-add, one reciprocal,
// one multiply-add instead of an exponential and a reciprocal.  Exact to ~1e-7 while |a|, |c| <= kExpTabLimit (both
// factors are normal f32 numbers; an overflowing product gives +1, an underflowing one -1, like tanh).  Beyond that
// the prep kernels raise a flag and the kernels evaluate fast_tanh(a + c) on the raw projections.
__device__ __forceinline__ float tanh_from_exp(float ea, float ec) {
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(fmaf(ea, ec, 1.0f));
}
// r = (1 - tanh(a + c)) / 2 = 1 / (1 + e^{2(a + c)}), the quantity joint_fwd_kernel puts on the matrix units (same tables, same
// saturation behaviour: 0 for an overflowing product, 1 for an underflowing one)
__device__ __forceinline__ float r_from_exp(float ea, float ec) { return __builtin_amdgcn_rcpf(fmaf(ea, ec, 1.0f)); }
__device__ __forceinline__ float fast_r(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * 2.8853900817779268f));
}

}  // namespace rnnt
