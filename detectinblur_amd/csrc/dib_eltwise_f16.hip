// The Half entry points of the epilogue family: dib_eltwise_vec.h's bias_act_kernel at 8 Half per lane, behind every convolution of
// the deblurrer under `--deblur_precision half` (models/deblur.py) and of its trainer under `--amp` (models/deblur_train.py; there also
// with the ReLU's sign mask).  It reproduces torch's Half ops in their order, each computed on upcast values and rounded once:
// half(y + b), relu(half(y + b)), half(half(y + b) + x).
#include <hip/hip_fp16.h>

#include "dib_eltwise_vec.h"

namespace dib {

// bias_act_kernel<F16Lane> for channel counts that are not a multiple of 8 or tensors that are not 16-byte aligned: the 3-channel
// outputs of the deblurrer's coarser scales (their bias add feeds conv_end)
template <bool RES, bool RELU>
__global__ __launch_bounds__(256) void bias_act_f16_scalar_kernel(__half *__restrict__ x, const float *__restrict__ bias,
                                                                 const __half *__restrict__ res, long long n, int C) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    float v = __half2float(x[i]) + bias[(int)(i % C)];
    if (RES) v = F16Lane::mid(v) + __half2float(res[i]);
    if (RELU) v = relu_keep_nan(v);
    x[i] = __float2half(v);
  }
}

}  // namespace dib

using namespace dib;

extern "C" int dib_bias_act_f16_nhwc(void *x_dev, const float *bias_dev, const void *residual_dev, long long n_elems, int C, int relu,
                                     void *stream) {
  const char *who = "dib_bias_act_f16_nhwc";
  if (n_elems < 0 || C <= 0 || (n_elems % C) != 0) { set_error("%s: n_elems must be a multiple of C", who); return DIB_EINVAL; }
  int code;
  if (!args_ok(who, n_elems == 0, {x_dev, bias_dev}, {}, &code)) return code;
  if ((((uintptr_t)x_dev | (uintptr_t)residual_dev) & 1) || ((uintptr_t)bias_dev & 3)) { set_error("%s: tensors must be aligned to their elements", who); return DIB_EINVAL; }
  if (C % 8 != 0 || misaligned({x_dev, bias_dev, residual_dev})) {
    auto scalar = residual_dev ? (relu ? bias_act_f16_scalar_kernel<true, true> : bias_act_f16_scalar_kernel<true, false>)
                               : (relu ? bias_act_f16_scalar_kernel<false, true> : bias_act_f16_scalar_kernel<false, false>);
    return launch(scalar, grid_1d(n_elems), stream, x_dev, bias_dev, residual_dev, n_elems, C);
  }
  // the sign-mask forms are dib_bias_act_mask_f16_nhwc's
  auto kernel = residual_dev ? (relu ? bias_act_kernel<F16Lane, true, true, false> : bias_act_kernel<F16Lane, true, false, false>)
                             : (relu ? bias_act_kernel<F16Lane, false, true, false> : bias_act_kernel<F16Lane, false, false, false>);
  return launch(kernel, grid_1d(n_elems / 8), stream, x_dev, bias_dev, residual_dev, n_elems / 8, C / 8, (unsigned char *)nullptr);
}

// The ReLU form with the sign mask of the STORED values, for the trainer under --amp (models/deblur_train.py): the same kernel, so the
// same bits as relu = 1 above.  Vector form only: the mask is one byte per 8-element lane vector.
extern "C" int dib_bias_act_mask_f16_nhwc(void *x_dev, const float *bias_dev, const void *residual_dev, long long n_elems, int C,
                                          unsigned char *mask_dev, void *stream) {
  const char *who = "dib_bias_act_mask_f16_nhwc";
  if (n_elems < 0 || C <= 0 || (C % 8) != 0 || (n_elems % C) != 0) { set_error("%s: needs C %% 8 == 0 and n_elems a multiple of C", who); return DIB_EINVAL; }
  int code;
  if (!args_ok(who, n_elems == 0, {x_dev, bias_dev, mask_dev}, {x_dev, bias_dev, residual_dev}, &code)) return code;
  return bias_act_launch<F16Lane>(x_dev, bias_dev, residual_dev, n_elems / 8, C / 8, 1, mask_dev, stream);
}
