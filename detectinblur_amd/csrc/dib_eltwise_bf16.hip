// bfloat16 entry points of the trunk's epilogue family: dib_eltwise_vec.h's kernels and wrappers at 8 bf16 per lane
// (dib_eltwise.hip holds the fp32 ones).  C % 8 == 0 and 16-byte aligned tensors throughout; the stem pool takes 4 channels per
// lane (C % 4 == 0), its convolution side is fp32.
#include "dib_eltwise_vec.h"

using namespace dib;

// Unlike the fp32 form there is no scalar kernel behind this one: other channel counts and unaligned tensors are refused.
static int bias_act_bf16(const char *who, void *x_dev, const float *bias_dev, const void *residual_dev, long long n_elems, int C, int relu,
                         unsigned char *mask_dev, void *stream) {
  if (n_elems < 0 || C <= 0 || (C % 8) != 0 || (n_elems % C) != 0) { set_error("%s: needs C %% 8 == 0 and n_elems a multiple of C", who); return DIB_EINVAL; }
  int code;
  if (!args_ok(who, n_elems == 0, {x_dev, bias_dev}, {x_dev, bias_dev, residual_dev}, &code)) return code;
  return bias_act_launch<Bf16Lane>(x_dev, bias_dev, residual_dev, n_elems / 8, C / 8, relu, mask_dev, stream);
}

extern "C" int dib_bias_act_bf16_nhwc(void *x_dev, const float *bias_dev, const void *residual_dev, long long n_elems, int C, int relu,
                                      void *stream) {
  return bias_act_bf16("dib_bias_act_bf16_nhwc", x_dev, bias_dev, residual_dev, n_elems, C, relu, nullptr, stream);
}

extern "C" int dib_bias_act_mask_bf16_nhwc(void *x_dev, const float *bias_dev, const void *residual_dev, long long n_elems, int C,
                                           unsigned char *mask_dev, void *stream) {
  if (!mask_dev) { set_error("dib_bias_act_mask_bf16_nhwc: null mask pointer"); return DIB_EINVAL; }
  return bias_act_bf16("dib_bias_act_mask_bf16_nhwc", x_dev, bias_dev, residual_dev, n_elems, C, 1, mask_dev, stream);
}

extern "C" int dib_relu_mask_backward_bf16(const void *grad_in_dev, const unsigned char *mask_dev, void *grad_out_dev, long long n_elems,
                                           void *stream) {
  return relu_mask_backward<Bf16Lane>("dib_relu_mask_backward_bf16", grad_in_dev, mask_dev, grad_out_dev, n_elems, stream);
}

extern "C" int dib_add_relu_mask_bf16(void *a_dev, const void *b_dev, const unsigned char *mask_dev, long long n_elems, void *stream) {
  return add_relu_mask<Bf16Lane>("dib_add_relu_mask_bf16", a_dev, b_dev, mask_dev, n_elems, stream);
}

extern "C" int dib_scatter_add_bf16_nhwc(void *a_dev, const void *b_dev, int N, int H, int W, int Hs, int Ws, int C, int stride, void *stream) {
  return scatter_add<Bf16Lane>("dib_scatter_add_bf16_nhwc", a_dev, b_dev, N, H, W, Hs, Ws, C, stride, stream);
}

extern "C" int dib_fpn_topdown_merge_bf16_nhwc(void *x_dev, const float *bias_dev, const void *top_dev, int N, int H, int W, int Ht, int Wt,
                                               int C, void *stream) {
  return topdown_merge<Bf16Lane>("dib_fpn_topdown_merge_bf16_nhwc", x_dev, bias_dev, top_dev, N, H, W, Ht, Wt, C, stream);
}

extern "C" int dib_stem_pool_forward_bf16(const float *x_dev, const float *bias_dev, void *out_dev, unsigned short *arg_dev, int N, int H, int W,
                                          int C, void *stream) {
  return stem_pool_forward<Bf16Lane>("dib_stem_pool_forward_bf16", x_dev, bias_dev, out_dev, arg_dev, N, H, W, C, stream);
}

extern "C" int dib_stem_pool_backward_bf16(const void *grad_out_dev, const unsigned short *arg_dev, float *grad_in_dev, int N, int H, int W, int C,
                                           void *stream) {
  return stem_pool_backward<Bf16Lane>("dib_stem_pool_backward_bf16", grad_out_dev, arg_dev, grad_in_dev, N, H, W, C, stream);
}
