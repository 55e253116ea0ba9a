// Internal: the total-variation factor of dib_rl_deconvolve_tv (csrc/dib_deconv_tv.hip), as dib_deconv.hip's iteration loop launches it.
#pragma once
#include "dib_common.h"

namespace dib {

constexpr float TV_LAMBDA_MAX = 0.1f;

// 0 < lambda <= 0.1, beta positive and finite (written so that a NaN fails)
inline bool tv_params_ok(float lambda, float beta) { return lambda > 0.f && lambda <= TV_LAMBDA_MAX && beta > 0.f && beta <= 3.4e38f; }

// out = x * g(x) per plane (include/dib.h: dib_tv_weight), x of `dtype` (DIB_F16 / DIB_F32), out fp32; one launch on `s`.  Arguments
// are the caller's to check: C, H, W >= 1, C H W < 2^31 - 1, tv_params_ok, no overlap.
int tv_weight_launch(const void *x, int dtype, float *out, int C, int H, int W, float lambda, float beta, hipStream_t s);

}  // namespace dib
