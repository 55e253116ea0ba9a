// fp32 entry points of the trunk's epilogue family (dib_eltwise_vec.h's kernels and wrappers at 4 fp32 per lane;
// dib_eltwise_bf16.hip holds the bf16 ones), and the fp32-only kernels around them: the scalar form of the bias epilogue, the
// frozen batch-norm folds, the bias epilogue with a layout change.
#include "dib_eltwise_vec.h"

namespace dib {

// bias_act_kernel for channel counts that are not a multiple of 4 or tensors that are not 16-byte aligned
template <bool RES, bool RELU>
__global__ __launch_bounds__(256) void bias_act_scalar_kernel(float *__restrict__ x, const float *__restrict__ bias,
                                                             const float *__restrict__ res, long long n, int C) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    float v = x[i] + bias[(int)(i % C)];
    if (RES) v += res[i];
    if (RELU) v = relu_keep_nan(v);
    x[i] = v;
  }
}


// ---- frozen batch-norm folds of many convolutions in ONE launch --------------------------------------------------------------
// Training folds every trunk convolution's frozen batch-norm into its weight each step (the weights move): per convolution
// that is five tiny launches forward (add eps, rsqrt, two multiplies, a subtract, the weight multiply) and one backward, 53
// times -- ~320 launches of ~5 us that the GPU waits for (profiles/r4_train_step_conv.txt).  Here: up to FOLD_MAX pairs per launch.
// Same operations in the same order as the tensor expressions (scale = bn_w * rsqrt(var + eps); shift = bn_b - mean * scale;
// wf = w * scale[co]), so the results are bit-identical to the per-convolution path (tests/test_detector_ops.py).
constexpr int FOLD_MAX = 32;
struct FoldArgs {
  const float *w[FOLD_MAX], *bn_w[FOLD_MAX], *bn_b[FOLD_MAX], *mean[FOLD_MAX], *var[FOLD_MAX];
  float *wf[FOLD_MAX], *scale[FOLD_MAX], *shift[FOLD_MAX];
  int inner[FOLD_MAX];            // elements per output channel (Ci * kh * kw)
  long long count[FOLD_MAX];      // Co * inner
  int block_start[FOLD_MAX + 1];  // first 1024-element block of pair k
  int n;
  float eps;
};

// pass 1: one thread per output channel.  torch's rsqrt kernel on this platform returns the correctly rounded value (checked
// against float(rsqrt(double(x))) on 200,000 samples, scratch/t_rsq.py) where rsqrtf() is v_rsq_f32's 1-ulp approximation
// (12 % of the samples differ): the double-precision form below reproduces torch's bits.
__global__ __launch_bounds__(256) void fold_scale_shift_kernel(FoldArgs a) {
#pragma clang fp contract(off)
  const int k = blockIdx.y;
  const int co = blockIdx.x * 256 + threadIdx.x;
  if (k >= a.n || (long long)co * a.inner[k] >= a.count[k]) return;
  const float v = a.var[k][co] + a.eps;
  const float sc = a.bn_w[k][co] * (float)(1.0 / sqrt((double)v));
  a.scale[k][co] = sc;
  a.shift[k][co] = a.bn_b[k][co] - a.mean[k][co] * sc;
}

// pass 2: wf = w * scale[co], 1024 consecutive elements of one weight per block
__global__ __launch_bounds__(256) void fold_bn_multi_kernel(FoldArgs a) {
#pragma clang fp contract(off)
  int k = 0;
  while (k + 1 < a.n && (int)blockIdx.x >= a.block_start[k + 1]) ++k;
  const long long base = (long long)((int)blockIdx.x - a.block_start[k]) * 1024;
  const int inner = a.inner[k];
  const float *w = a.w[k];
  const float *sc = a.scale[k];
  float *wf = a.wf[k];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long e = base + j * 256 + threadIdx.x;
    if (e >= a.count[k]) break;
    wf[e] = w[e] * sc[(int)(e / inner)];
  }
}

struct ScaleRowsArgs {
  const float *g[FOLD_MAX], *scale[FOLD_MAX];
  float *dw[FOLD_MAX];
  int inner[FOLD_MAX];
  long long count[FOLD_MAX];
  int block_start[FOLD_MAX + 1];
  int n;
};

__global__ __launch_bounds__(256) void scale_rows_multi_kernel(ScaleRowsArgs a) {
  int k = 0;
  while (k + 1 < a.n && (int)blockIdx.x >= a.block_start[k + 1]) ++k;
  const long long base = (long long)((int)blockIdx.x - a.block_start[k]) * 1024;
  const int inner = a.inner[k];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long e = base + j * 256 + threadIdx.x;
    if (e >= a.count[k]) break;
    a.dw[k][e] = a.g[k][e] * a.scale[k][(int)(e / inner)];
  }
}

}  // namespace dib

using namespace dib;

// x_dev: [n_elems] fp32 viewed as [..., C] with the channel fastest (NHWC storage), updated in place:
//   x = act(x + bias[c] (+ residual)),  act = ReLU when relu != 0.
static int bias_act_impl(float *x_dev, const float *bias_dev, const float *residual_dev, long long n_elems, int C, int relu,
                         unsigned char *mask_dev, void *stream) {
  if (n_elems < 0 || C <= 0 || (n_elems % C) != 0) { set_error("dib_bias_act_nhwc: n_elems must be a multiple of C"); return DIB_EINVAL; }
  int code;
  if (!args_ok("dib_bias_act_nhwc", n_elems == 0, {x_dev, bias_dev}, {}, &code)) return code;
  if (C % 4 == 0 && !misaligned({x_dev, bias_dev, residual_dev}))
    return bias_act_launch<F32Lane>(x_dev, bias_dev, residual_dev, n_elems / 4, C / 4, relu, mask_dev, stream);
  auto kernel = residual_dev ? (relu ? bias_act_scalar_kernel<true, true> : bias_act_scalar_kernel<true, false>)
                             : (relu ? bias_act_scalar_kernel<false, true> : bias_act_scalar_kernel<false, false>);
  return launch(kernel, grid_1d(n_elems), stream, x_dev, bias_dev, residual_dev, n_elems, C);
}

extern "C" int dib_bias_act_nhwc(float *x_dev, const float *bias_dev, const float *residual_dev, long long n_elems, int C,
                                 int relu, void *stream) {
  return bias_act_impl(x_dev, bias_dev, residual_dev, n_elems, C, relu, nullptr, stream);
}

// Same, and mask_dev[n_elems / 4] receives the sign pattern of the result (one byte per 4 consecutive elements, bit k =
// element 4i + k > 0): dib_relu_mask_backward's input.  Needs C % 4 == 0 and 16-byte aligned pointers.
extern "C" int dib_bias_act_mask_nhwc(float *x_dev, const float *bias_dev, const float *residual_dev, long long n_elems, int C,
                                      unsigned char *mask_dev, void *stream) {
  if (!mask_dev) { set_error("dib_bias_act_mask_nhwc: null mask pointer"); return DIB_EINVAL; }
  if ((C % 4) != 0 || misaligned({x_dev, bias_dev, residual_dev})) {
    set_error("dib_bias_act_mask_nhwc: needs C %% 4 == 0 and 16-byte aligned tensors");
    return DIB_EINVAL;
  }
  return bias_act_impl(x_dev, bias_dev, residual_dev, n_elems, C, 1, mask_dev, stream);
}

// grad_out = mask ? grad_in : 0 over n_elems fp32 values (n_elems % 4 == 0, 16-byte aligned; grad_out may alias grad_in).
extern "C" int dib_relu_mask_backward(const float *grad_in_dev, const unsigned char *mask_dev, float *grad_out_dev, long long n_elems,
                                      void *stream) {
  return relu_mask_backward<F32Lane>("dib_relu_mask_backward", grad_in_dev, mask_dev, grad_out_dev, n_elems, stream);
}

// a = (a + b), then zeroed where the mask bit is clear (mask_dev NULL: plain accumulate).  n_elems % 4 == 0, 16-byte aligned.
extern "C" int dib_add_relu_mask(float *a_dev, const float *b_dev, const unsigned char *mask_dev, long long n_elems, void *stream) {
  return add_relu_mask<F32Lane>("dib_add_relu_mask", a_dev, b_dev, mask_dev, n_elems, stream);
}

// a[N, H, W, C] (channels-last fp32) += b[N, Hs, Ws, C] at the pixels (ys * stride, xs * stride); C % 4 == 0, 16-byte aligned.
extern "C" int dib_scatter_add_nhwc(float *a_dev, const float *b_dev, int N, int H, int W, int Hs, int Ws, int C, int stride, void *stream) {
  return scatter_add<F32Lane>("dib_scatter_add_nhwc", a_dev, b_dev, N, H, W, Hs, Ws, C, stride, stream);
}

// x[N, H, W, C] (channels-last fp32, in place) += bias[C] + top[N, Ht, Wt, C] at the nearest-neighbour source pixel;
// C % 4 == 0, 16-byte aligned.
extern "C" int dib_fpn_topdown_merge_nhwc(float *x_dev, const float *bias_dev, const float *top_dev, int N, int H, int W, int Ht, int Wt,
                                          int C, void *stream) {
  return topdown_merge<F32Lane>("dib_fpn_topdown_merge_nhwc", x_dev, bias_dev, top_dev, N, H, W, Ht, Wt, C, stream);
}

// out[N, Ho, Wo, C] = max_pool2d(relu(x[N, H, W, C] + bias[C]), 3, stride 2, padding 1), Ho = (H - 1) / 2 + 1; arg: one
// unsigned short per 4 output channels (4-bit window position of the winner per channel, 15 = no gradient).  C % 4 == 0.
extern "C" int dib_stem_pool_forward(const float *x_dev, const float *bias_dev, float *out_dev, unsigned short *arg_dev, int N, int H, int W,
                                     int C, void *stream) {
  return stem_pool_forward<F32Lane>("dib_stem_pool_forward", x_dev, bias_dev, out_dev, arg_dev, N, H, W, C, stream);
}

// grad_in[N, H, W, C] from grad_out[N, Ho, Wo, C] and the forward pass's arg.
extern "C" int dib_stem_pool_backward(const float *grad_out_dev, const unsigned short *arg_dev, float *grad_in_dev, int N, int H, int W, int C,
                                      void *stream) {
  return stem_pool_backward<F32Lane>("dib_stem_pool_backward", grad_out_dev, arg_dev, grad_in_dev, N, H, W, C, stream);
}

// Frozen batch-norm folds of n convolutions (any n; FOLD_MAX pairs per launch).  Host arrays of n device pointers / sizes:
// w[k] [Co[k]][inner[k]] dense with the output channel outermost (contiguous OR channels-last weights), bn_* [Co[k]];
// wf[k] receives the folded weight in w[k]'s element order, scale[k] / shift[k] [Co[k]].
extern "C" int dib_fold_bn_multi(const float *const *w, const float *const *bn_w, const float *const *bn_b, const float *const *mean,
                                 const float *const *var, const int *Co, const int *inner, int n, float eps, float *const *wf,
                                 float *const *scale, float *const *shift, void *stream) {
  if (n < 0 || (n > 0 && (!w || !bn_w || !bn_b || !mean || !var || !Co || !inner || !wf || !scale || !shift))) { set_error("dib_fold_bn_multi: null pointer or negative count"); return DIB_EINVAL; }
  for (int k0 = 0; k0 < n; k0 += FOLD_MAX) {
    FoldArgs a;
    a.n = n - k0 < FOLD_MAX ? n - k0 : FOLD_MAX;
    a.eps = eps;
    int blocks = 0;
    for (int i = 0; i < a.n; ++i) {
      const int k = k0 + i;
      if (!w[k] || !bn_w[k] || !bn_b[k] || !mean[k] || !var[k] || !wf[k] || !scale[k] || !shift[k] || Co[k] <= 0 || inner[k] <= 0) { set_error("dib_fold_bn_multi: pair %d has a null pointer or an empty shape", k); return DIB_EINVAL; }
      a.w[i] = w[k]; a.bn_w[i] = bn_w[k]; a.bn_b[i] = bn_b[k]; a.mean[i] = mean[k]; a.var[i] = var[k];
      a.wf[i] = wf[k]; a.scale[i] = scale[k]; a.shift[i] = shift[k];
      a.inner[i] = inner[k]; a.count[i] = (long long)Co[k] * inner[k];
      a.block_start[i] = blocks;
      blocks += (int)((a.count[i] + 1023) / 1024);
    }
    for (int i = a.n; i <= FOLD_MAX; ++i) a.block_start[i] = blocks;
    int max_co = 0;
    for (int i = 0; i < a.n; ++i) max_co = Co[k0 + i] > max_co ? Co[k0 + i] : max_co;
    hipLaunchKernelGGL(fold_scale_shift_kernel, dim3((unsigned)((max_co + 255) / 256), (unsigned)a.n), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(fold_bn_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  }
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

// The backward of those folds: dw[k][co][...] = g[k][co][...] * scale[k][co] (the gradient of w * scale[co] with respect to w).
extern "C" int dib_scale_rows_multi(const float *const *g, const float *const *scale, const int *Co, const int *inner, int n,
                                    float *const *dw, void *stream) {
  if (n < 0 || (n > 0 && (!g || !scale || !Co || !inner || !dw))) { set_error("dib_scale_rows_multi: null pointer or negative count"); return DIB_EINVAL; }
  for (int k0 = 0; k0 < n; k0 += FOLD_MAX) {
    ScaleRowsArgs a;
    a.n = n - k0 < FOLD_MAX ? n - k0 : FOLD_MAX;
    int blocks = 0;
    for (int i = 0; i < a.n; ++i) {
      const int k = k0 + i;
      if (!g[k] || !scale[k] || !dw[k] || Co[k] <= 0 || inner[k] <= 0) { set_error("dib_scale_rows_multi: tensor %d has a null pointer or an empty shape", k); return DIB_EINVAL; }
      a.g[i] = g[k]; a.scale[i] = scale[k]; a.dw[i] = dw[k];
      a.inner[i] = inner[k]; a.count[i] = (long long)Co[k] * inner[k];
      a.block_start[i] = blocks;
      blocks += (int)((a.count[i] + 1023) / 1024);
    }
    for (int i = a.n; i <= FOLD_MAX; ++i) a.block_start[i] = blocks;
    hipLaunchKernelGGL(scale_rows_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  }
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

// ---- bias (+ ReLU) with the layout change MIOpen's planar kernels need, in one pass ------------------------------------------------
// At batch 1 the wide 3x3 convolutions of ResNet layer2-4 run 1.4-1.7x faster through MIOpen's planar (NCHW) kernels than through
// its channels-last ones (models/backbone.py: _as_planar).  Around each of them eager PyTorch spent four passes: the epilogue of the
// convolution before (in place, channels-last), a copy to planar, a copy of the result back to channels-last, its epilogue
// (profiles/r4_trunk_b1_trace.txt: 0.68 ms of copies per image, the strided NHWC -> NCHW copy at 0.6 TB/s).  These are the two
// middle pairs as one pass each: a 64 x 64 tile transpose through LDS with the bias indexed on the channel axis.
//   to_planar = 1: in [N][HW][C] -> out [N][C][HW];   to_planar = 0: in [N][C][HW] -> out [N][HW][C].   out = act(in + bias[c])
namespace dib {

template <bool RELU>
__global__ __launch_bounds__(256) void bias_act_transpose_kernel(const float *__restrict__ in, const float *__restrict__ bias, float *__restrict__ out,
                                                                int rows, int cols, int bias_on_cols) {
  // in: [rows][cols] per image, out: [cols][rows]
  __shared__ float tile[64][65];
  const size_t img = (size_t)blockIdx.z * rows * cols;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;      // 64 x 4
  const int c = c0 + tx;
  const float bc = (bias_on_cols && c < cols) ? bias[c] : 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int r = r0 + ty + 4 * k;
    if (r < rows && c < cols) {
      float v = in[img + (size_t)r * cols + c] + (bias_on_cols ? bc : bias[r]);
      if (RELU) v = relu_keep_nan(v);                            // as bias_act_kernel
      tile[ty + 4 * k][tx] = v;
    }
  }
  __syncthreads();
  const int orow = r0 + tx;                                     // output: [cols][rows]: consecutive lanes along `rows`
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int oc = c0 + ty + 4 * k;
    if (oc < cols && orow < rows) out[img + (size_t)oc * rows + orow] = tile[tx][ty + 4 * k];
  }
}

}  // namespace dib

extern "C" int dib_bias_act_transpose(const float *in_dev, const float *bias_dev, float *out_dev, int N, int C, long long HW, int to_planar, int relu,
                                      void *stream) {
  if (N < 0 || C <= 0 || HW <= 0 || HW > 0x7fffffffLL) { set_error("dib_bias_act_transpose: bad shape"); return DIB_EINVAL; }
  if (N == 0) return DIB_OK;
  if (!in_dev || !bias_dev || !out_dev || in_dev == out_dev) { set_error("dib_bias_act_transpose: null or aliased pointers"); return DIB_EINVAL; }
  const int rows = to_planar ? (int)HW : C, cols = to_planar ? C : (int)HW;
  const dim3 grid((cols + 63) / 64, (rows + 63) / 64, N);
  if (grid.y > 65535 || grid.z > 65535) { set_error("dib_bias_act_transpose: tensor too large for one launch"); return DIB_EINVAL; }
  if (relu) hipLaunchKernelGGL(dib::bias_act_transpose_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, in_dev, bias_dev, out_dev, rows, cols, to_planar);
  else hipLaunchKernelGGL(dib::bias_act_transpose_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, in_dev, bias_dev, out_dev, rows, cols, to_planar);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}
