// bfloat16 forms of the trunk's epilogue family (dib_eltwise.hip holds the fp32 ones): channels-last activations stored as
// bf16, per-channel vectors (bias, folded shift) read as fp32.  Every kernel upcasts, does the fp32 kernel's arithmetic in its
// order, and rounds ONCE (to nearest even) at the store, so each is checkable bit for bit against the torch expression
// evaluated in fp32 and cast once (tests/test_amp_gpu.py).  8 elements per lane: every load and store of an activation is
// 16 bytes wide (C % 8 == 0, 16-byte aligned tensors; every trunk width is a multiple of 64).  No atomics, no scratch.
#include "dib_common.h"

namespace dib {

typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
// two fp32 -> two bf16 in one word, round to nearest even (v_cvt_pk_bf16_f32 on gfx950); NaN stays NaN, +-inf stays
__device__ __forceinline__ unsigned bf_pack(float a, float b) {
  const f32x2_t v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
__device__ __forceinline__ void bf_unpack8(const uint4 u, float v[8]) {
  v[0] = bf_lo(u.x); v[1] = bf_hi(u.x); v[2] = bf_lo(u.y); v[3] = bf_hi(u.y);
  v[4] = bf_lo(u.z); v[5] = bf_hi(u.z); v[6] = bf_lo(u.w); v[7] = bf_hi(u.w);
}
__device__ __forceinline__ uint4 bf_pack8(const float v[8]) {
  return make_uint4(bf_pack(v[0], v[1]), bf_pack(v[2], v[3]), bf_pack(v[4], v[5]), bf_pack(v[6], v[7]));
}
// torch's relu (clamp_min): a NaN goes through
__device__ __forceinline__ float relu_nan(float v) { return v != v ? v : fmaxf(v, 0.f); }
// bit k = stored bf16 element k of the 8 is > 0 (the value AFTER rounding: a positive fp32 below half of bf16's smallest
// denormal is stored as zero and gets no gradient, as in the plain graph on the stored tensor)
__device__ __forceinline__ unsigned sign_mask8(const uint4 u) {
  float v[8];
  bf_unpack8(u, v);
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) m |= (v[k] > 0.f ? 1u : 0u) << k;
  return m;
}
// keep the halves of the four words whose mask bit is set (cleared ones become +0, torch's threshold_backward)
__device__ __forceinline__ uint4 select8(const uint4 u, unsigned m) {
  auto keep = [](unsigned w, unsigned b) { return w & (((b & 1u) ? 0xffffu : 0u) | ((b & 2u) ? 0xffff0000u : 0u)); };
  return make_uint4(keep(u.x, m), keep(u.y, m >> 2), keep(u.z, m >> 4), keep(u.w, m >> 6));
}

// x = bf16(act(float(x) + bias[c] (+ float(res)))) in place; MASK: one byte per 8 elements.
template <bool RES, bool RELU, bool MASK>
__global__ __launch_bounds__(256) void bias_act_bf16_kernel(uint4 *__restrict__ x, const float4 *__restrict__ bias,
                                                           const uint4 *__restrict__ res, long long n8, int C8,
                                                           unsigned char *__restrict__ mask) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
    float v[8];
    bf_unpack8(x[i], v);
    const int c = (int)(i % C8) * 2;
    const float4 b0 = bias[c], b1 = bias[c + 1];
    v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w; v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
    if (RES) {
      float r[8];
      bf_unpack8(res[i], r);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] += r[k];
    }
    if (RELU) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = relu_nan(v[k]);
    }
    const uint4 o = bf_pack8(v);
    x[i] = o;
    if (MASK) mask[i] = (unsigned char)sign_mask8(o);
  }
}

__global__ __launch_bounds__(256) void relu_mask_bwd_bf16_kernel(const uint4 *__restrict__ g, const unsigned char *__restrict__ mask,
                                                                uint4 *__restrict__ out, long long n8) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x)
    out[i] = select8(g[i], mask[i]);
}

// a = bf16(float(a) + float(b)) [then zeroed where the mask bit is clear]
template <bool MASK>
__global__ __launch_bounds__(256) void add_mask_bf16_kernel(uint4 *__restrict__ a, const uint4 *__restrict__ b,
                                                           const unsigned char *__restrict__ mask, long long n8) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
    float v[8], w[8];
    bf_unpack8(a[i], v);
    bf_unpack8(b[i], w);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] += w[k];
    uint4 o = bf_pack8(v);
    if (MASK) o = select8(o, mask[i]);
    a[i] = o;
  }
}

// a[n, ys * s, xs * s, :] = bf16(float(a) + float(b[n, ys, xs, :]))
__global__ __launch_bounds__(256) void scatter_add_bf16_kernel(uint4 *__restrict__ a, const uint4 *__restrict__ b, int Hs, int Ws, int C8,
                                                              int H, int W, int s, long long n8) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C8);
    long long p = i / C8;
    const int xs = (int)(p % Ws);
    p /= Ws;
    const int ys = (int)(p % Hs);
    const long long n = p / Hs;
    const long long j = ((n * H + (long long)ys * s) * W + (long long)xs * s) * C8 + c;
    float v[8], w[8];
    bf_unpack8(a[j], v);
    bf_unpack8(b[i], w);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] += w[k];
    a[j] = bf_pack8(v);
  }
}

// x[n, h, w, :] = bf16((float(x) + bias[:]) + float(top[n, sh(h), sw(w), :])): the fp32 kernel's expression in its order
__global__ __launch_bounds__(256) void topdown_merge_bf16_kernel(uint4 *__restrict__ x, const float4 *__restrict__ bias,
                                                                const uint4 *__restrict__ top, int H, int W, int Ht, int Wt, int C8,
                                                                float scale_h, float scale_w, long long n8) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C8);
    long long p = i / C8;
    const int w = (int)(p % W);
    p /= W;
    const int h = (int)(p % H);
    const long long n = p / H;
    const int sh = min((int)floorf((float)h * scale_h), Ht - 1), sw = min((int)floorf((float)w * scale_w), Wt - 1);
    float v[8], t[8];
    bf_unpack8(x[i], v);
    bf_unpack8(top[((n * Ht + sh) * Wt + sw) * C8 + c], t);
    const float4 b0 = bias[2 * c], b1 = bias[2 * c + 1];
    v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w; v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] += t[k];
    x[i] = bf_pack8(v);
  }
}

// ResNet stem behind the fp32 7x7 convolution (3 input channels: it stays an fp32 convolution, models/backbone.py): the fp32
// kernel's pool of relu(x + bias) -- same window order, same strict `>`, same `arg` -- with the pooled maximum rounded once to
// bf16 at the store.  Rounding is monotonic, so the recorded winner is also a maximum of the rounded values.  4 channels per
// lane: 16-byte loads of the fp32 input, 8-byte stores.
__global__ __launch_bounds__(256) void stem_pool_fwd_bf16_kernel(const float4 *__restrict__ x, const float4 *__restrict__ bias,
                                                                uint2 *__restrict__ out, unsigned short *__restrict__ arg, int H, int W,
                                                                int Ho, int Wo, int C4) {
  const unsigned col = blockIdx.x * 256u + threadIdx.x;
  if (col >= (unsigned)(Wo * C4)) return;
  const int ow = (int)(col / (unsigned)C4), c = (int)(col % (unsigned)C4), oh = blockIdx.y;
  const size_t n = blockIdx.z;
  const float4 b = bias[c];
  const float ninf = -__builtin_inff();
  float4 m = make_float4(ninf, ninf, ninf, ninf);
  unsigned ax = 15, ay = 15, az = 15, aw = 15;
  float4 v[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int h = oh * 2 - 1 + k / 3, w = ow * 2 - 1 + k % 3;
    const int hc = min(max(h, 0), H - 1), wc = min(max(w, 0), W - 1);
    v[k] = x[((n * H + hc) * W + wc) * C4 + c];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int h = oh * 2 - 1 + k / 3, w = ow * 2 - 1 + k % 3;
    const bool in = h >= 0 && h < H && w >= 0 && w < W;
    const float vx = in ? v[k].x + b.x : ninf, vy = in ? v[k].y + b.y : ninf, vz = in ? v[k].z + b.z : ninf, vw = in ? v[k].w + b.w : ninf;
    if (vx > m.x) { m.x = vx; ax = k; }
    if (vy > m.y) { m.y = vy; ay = k; }
    if (vz > m.z) { m.z = vz; az = k; }
    if (vw > m.w) { m.w = vw; aw = k; }
  }
  if (!(m.x > 0.f)) { m.x = 0.f; ax = 15; }
  if (!(m.y > 0.f)) { m.y = 0.f; ay = 15; }
  if (!(m.z > 0.f)) { m.z = 0.f; az = 15; }
  if (!(m.w > 0.f)) { m.w = 0.f; aw = 15; }
  const size_t i = ((n * Ho + oh) * Wo) * C4 + col;
  out[i] = make_uint2(bf_pack(m.x, m.y), bf_pack(m.z, m.w));
  arg[i] = (unsigned short)(ax | (ay << 4) | (az << 8) | (aw << 12));
}

// Its backward: bf16 pooled gradient + arg in, the fp32 convolution's dense fp32 gradient out.  An input pixel takes the pooled
// gradient of up to four windows: summed in fp32 in the fp32 kernel's order, nothing is rounded.
__global__ __launch_bounds__(256) void stem_pool_bwd_bf16_kernel(const uint2 *__restrict__ g_out, const unsigned short *__restrict__ arg,
                                                                float4 *__restrict__ g_in, int H, int W, int Ho, int Wo, int C4) {
  const unsigned col = blockIdx.x * 256u + threadIdx.x;
  if (col >= (unsigned)(W * C4)) return;
  const int w = (int)(col / (unsigned)C4), c = (int)(col % (unsigned)C4), h = blockIdx.y;
  const size_t n = blockIdx.z;
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  const int ohs[2] = {h >> 1, (h + 1) >> 1}, ows[2] = {w >> 1, (w + 1) >> 1};
  unsigned a[4];
  uint2 go[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int oh = min(ohs[q >> 1], Ho - 1), ow = min(ows[q & 1], Wo - 1);
    const size_t j = ((n * Ho + oh) * Wo + ow) * C4 + c;
    a[q] = arg[j];
    go[q] = g_out[j];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int oh = ohs[q >> 1], ow = ows[q & 1];
    const bool use = oh < Ho && ow < Wo && ((q >> 1) == 0 || ohs[1] != ohs[0]) && ((q & 1) == 0 || ows[1] != ows[0]);
    const unsigned k = use ? (unsigned)(h - (oh * 2 - 1)) * 3u + (unsigned)(w - (ow * 2 - 1)) : 14u;      // 14: never recorded
    if ((a[q] & 15u) == k) g.x += bf_lo(go[q].x);
    if (((a[q] >> 4) & 15u) == k) g.y += bf_hi(go[q].x);
    if (((a[q] >> 8) & 15u) == k) g.z += bf_lo(go[q].y);
    if ((a[q] >> 12) == k) g.w += bf_hi(go[q].y);
  }
  g_in[((n * H + h) * W) * C4 + col] = g;
}

static inline unsigned stream_blocks(long long n) {
  const long long blocks = (n + 255) / 256;
  return (unsigned)(blocks > (1ll << 30) ? (1ll << 30) : blocks);
}
static inline bool misaligned(const void *a, const void *b = nullptr, const void *c = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) != 0;
}

static int bias_act_bf16_impl(const char *who, void *x_dev, const float *bias_dev, const void *residual_dev, long long n_elems, int C, int relu,
                              unsigned char *mask_dev, void *stream) {
  if (n_elems < 0 || C <= 0 || (C % 8) != 0 || (n_elems % C) != 0) { set_error("%s: needs C %% 8 == 0 and n_elems a multiple of C", who); return DIB_EINVAL; }
  if (n_elems == 0) return DIB_OK;
  if (!x_dev || !bias_dev) { set_error("%s: null pointer", who); return DIB_EINVAL; }
  if (misaligned(x_dev, bias_dev, residual_dev)) { set_error("%s: tensors must be 16-byte aligned", who); return DIB_EINVAL; }
  const long long n8 = n_elems / 8;
  const dim3 grid(stream_blocks(n8));
  hipStream_t s = (hipStream_t)stream;
#define DIB_LAUNCH(RES, RELU, MASK)                                                                                                 \
  hipLaunchKernelGGL((bias_act_bf16_kernel<RES, RELU, MASK>), grid, dim3(256), 0, s, (uint4 *)x_dev, (const float4 *)bias_dev, \
                     (const uint4 *)residual_dev, n8, C / 8, mask_dev)
  if (mask_dev) { if (residual_dev) DIB_LAUNCH(true, true, true); else DIB_LAUNCH(false, true, true); }
  else if (residual_dev) { if (relu) DIB_LAUNCH(true, true, false); else DIB_LAUNCH(true, false, false); }
  else { if (relu) DIB_LAUNCH(false, true, false); else DIB_LAUNCH(false, false, false); }
#undef DIB_LAUNCH
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

}  // namespace dib

using namespace dib;

extern "C" int dib_bias_act_bf16_nhwc(void *x_dev, const float *bias_dev, const void *residual_dev, long long n_elems, int C, int relu,
                                      void *stream) {
  return bias_act_bf16_impl("dib_bias_act_bf16_nhwc", x_dev, bias_dev, residual_dev, n_elems, C, relu, nullptr, stream);
}

extern "C" int dib_bias_act_mask_bf16_nhwc(void *x_dev, const float *bias_dev, const void *residual_dev, long long n_elems, int C,
                                           unsigned char *mask_dev, void *stream) {
  if (!mask_dev) { set_error("dib_bias_act_mask_bf16_nhwc: null mask pointer"); return DIB_EINVAL; }
  return bias_act_bf16_impl("dib_bias_act_mask_bf16_nhwc", x_dev, bias_dev, residual_dev, n_elems, C, 1, mask_dev, stream);
}

extern "C" int dib_relu_mask_backward_bf16(const void *grad_in_dev, const unsigned char *mask_dev, void *grad_out_dev, long long n_elems,
                                           void *stream) {
  if (n_elems < 0 || (n_elems % 8) != 0) { set_error("dib_relu_mask_backward_bf16: n_elems must be a non-negative multiple of 8"); return DIB_EINVAL; }
  if (n_elems == 0) return DIB_OK;
  if (!grad_in_dev || !mask_dev || !grad_out_dev) { set_error("dib_relu_mask_backward_bf16: null pointer"); return DIB_EINVAL; }
  if (misaligned(grad_in_dev, grad_out_dev)) { set_error("dib_relu_mask_backward_bf16: tensors must be 16-byte aligned"); return DIB_EINVAL; }
  const long long n8 = n_elems / 8;
  hipLaunchKernelGGL(relu_mask_bwd_bf16_kernel, dim3(stream_blocks(n8)), dim3(256), 0, (hipStream_t)stream, (const uint4 *)grad_in_dev, mask_dev,
                     (uint4 *)grad_out_dev, n8);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

extern "C" int dib_add_relu_mask_bf16(void *a_dev, const void *b_dev, const unsigned char *mask_dev, long long n_elems, void *stream) {
  if (n_elems < 0 || (n_elems % 8) != 0) { set_error("dib_add_relu_mask_bf16: n_elems must be a non-negative multiple of 8"); return DIB_EINVAL; }
  if (n_elems == 0) return DIB_OK;
  if (!a_dev || !b_dev) { set_error("dib_add_relu_mask_bf16: null pointer"); return DIB_EINVAL; }
  if (misaligned(a_dev, b_dev)) { set_error("dib_add_relu_mask_bf16: tensors must be 16-byte aligned"); return DIB_EINVAL; }
  const long long n8 = n_elems / 8;
  const dim3 grid(stream_blocks(n8));
  if (mask_dev) hipLaunchKernelGGL(add_mask_bf16_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (uint4 *)a_dev, (const uint4 *)b_dev, mask_dev, n8);
  else hipLaunchKernelGGL(add_mask_bf16_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (uint4 *)a_dev, (const uint4 *)b_dev, (const unsigned char *)nullptr, n8);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

extern "C" int dib_scatter_add_bf16_nhwc(void *a_dev, const void *b_dev, int N, int H, int W, int Hs, int Ws, int C, int stride, void *stream) {
  if (N < 0 || H <= 0 || W <= 0 || Hs <= 0 || Ws <= 0 || C <= 0 || (C % 8) != 0 || stride < 1) { set_error("dib_scatter_add_bf16_nhwc: bad shape (C %% 8 == 0)"); return DIB_EINVAL; }
  if ((long long)(Hs - 1) * stride > H - 1 || (long long)(Ws - 1) * stride > W - 1) { set_error("dib_scatter_add_bf16_nhwc: strided grid leaves the target"); return DIB_ESHAPE; }
  if (N == 0) return DIB_OK;
  if (!a_dev || !b_dev) { set_error("dib_scatter_add_bf16_nhwc: null pointer"); return DIB_EINVAL; }
  if (misaligned(a_dev, b_dev)) { set_error("dib_scatter_add_bf16_nhwc: tensors must be 16-byte aligned"); return DIB_EINVAL; }
  const long long n8 = (long long)N * Hs * Ws * (C / 8);
  hipLaunchKernelGGL(scatter_add_bf16_kernel, dim3(stream_blocks(n8)), dim3(256), 0, (hipStream_t)stream, (uint4 *)a_dev, (const uint4 *)b_dev, Hs, Ws,
                     C / 8, H, W, stride, n8);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

extern "C" int dib_fpn_topdown_merge_bf16_nhwc(void *x_dev, const float *bias_dev, const void *top_dev, int N, int H, int W, int Ht, int Wt,
                                               int C, void *stream) {
  if (N < 0 || H <= 0 || W <= 0 || Ht <= 0 || Wt <= 0 || C <= 0 || (C % 8) != 0) { set_error("dib_fpn_topdown_merge_bf16_nhwc: bad shape (C %% 8 == 0)"); return DIB_EINVAL; }
  if (N == 0) return DIB_OK;
  if (!x_dev || !bias_dev || !top_dev) { set_error("dib_fpn_topdown_merge_bf16_nhwc: null pointer"); return DIB_EINVAL; }
  if (misaligned(x_dev, bias_dev, top_dev)) { set_error("dib_fpn_topdown_merge_bf16_nhwc: tensors must be 16-byte aligned"); return DIB_EINVAL; }
  const long long n8 = (long long)N * H * W * (C / 8);
  hipLaunchKernelGGL(topdown_merge_bf16_kernel, dim3(stream_blocks(n8)), dim3(256), 0, (hipStream_t)stream, (uint4 *)x_dev, (const float4 *)bias_dev,
                     (const uint4 *)top_dev, H, W, Ht, Wt, C / 8, (float)Ht / (float)H, (float)Wt / (float)W, n8);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

extern "C" int dib_stem_pool_forward_bf16(const float *x_dev, const float *bias_dev, void *out_dev, unsigned short *arg_dev, int N, int H, int W,
                                          int C, void *stream) {
  if (N < 0 || H <= 0 || W <= 0 || C <= 0 || (C % 4) != 0) { set_error("dib_stem_pool_forward_bf16: bad shape (C %% 4 == 0)"); return DIB_EINVAL; }
  if (N == 0) return DIB_OK;
  if (!x_dev || !bias_dev || !out_dev || !arg_dev) { set_error("dib_stem_pool_forward_bf16: null pointer"); return DIB_EINVAL; }
  if (misaligned(x_dev, bias_dev, out_dev)) { set_error("dib_stem_pool_forward_bf16: tensors must be 16-byte aligned"); return DIB_EINVAL; }
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  if (Ho > 65535 || N > 65535) { set_error("dib_stem_pool_forward_bf16: at most 65535 pooled rows and images per call"); return DIB_ESHAPE; }
  hipLaunchKernelGGL(stem_pool_fwd_bf16_kernel, dim3((unsigned)((Wo * (C / 4) + 255) / 256), (unsigned)Ho, (unsigned)N), dim3(256), 0, (hipStream_t)stream,
                     (const float4 *)x_dev, (const float4 *)bias_dev, (uint2 *)out_dev, arg_dev, H, W, Ho, Wo, C / 4);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

extern "C" int dib_stem_pool_backward_bf16(const void *grad_out_dev, const unsigned short *arg_dev, float *grad_in_dev, int N, int H, int W, int C,
                                           void *stream) {
  if (N < 0 || H <= 0 || W <= 0 || C <= 0 || (C % 4) != 0) { set_error("dib_stem_pool_backward_bf16: bad shape (C %% 4 == 0)"); return DIB_EINVAL; }
  if (N == 0) return DIB_OK;
  if (!grad_out_dev || !arg_dev || !grad_in_dev) { set_error("dib_stem_pool_backward_bf16: null pointer"); return DIB_EINVAL; }
  if (misaligned(grad_out_dev, grad_in_dev)) { set_error("dib_stem_pool_backward_bf16: tensors must be 16-byte aligned"); return DIB_EINVAL; }
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  if (H > 65535 || N > 65535) { set_error("dib_stem_pool_backward_bf16: at most 65535 rows and images per call"); return DIB_ESHAPE; }
  hipLaunchKernelGGL(stem_pool_bwd_bf16_kernel, dim3((unsigned)((W * (C / 4) + 255) / 256), (unsigned)H, (unsigned)N), dim3(256), 0, (hipStream_t)stream,
                     (const uint2 *)grad_out_dev, arg_dev, (float4 *)grad_in_dev, H, W, Ho, Wo, C / 4);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}
