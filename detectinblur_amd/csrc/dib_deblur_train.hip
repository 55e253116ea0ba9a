// What the DeepDeblur trainer (detectinblur_amd/train_deblurrer.py, models/deblur_train.py) runs around MIOpen's convolutions that
// the inference stage (dib_deblur.hip, dib_eltwise.hip) does not already have.  Three HBM-bound streams; no scratch, no float
// atomics, no host synchronisation, everything on the caller's stream (capturable).
//
//   (a) patches_kernel       one random patch per image of a ragged list, with DeepDeblur's augmentation (crop, hflip, vflip,
//                            transpose, channel order): pure data movement, one launch for the batch.  One output element per lane:
//                            stores are consecutive; loads are consecutive too unless the patch is transposed (then they stride by
//                            a source row -- 6 MB per batch at the defaults, against the step's gigabytes of activations).
//   (b) bias_grad_partial_kernel + bias_grad_final_kernel
//                            backward of the convolution epilogue: grad_out = mask bit ? grad_in : 0 (relu_mask_bwd_kernel's
//                            select, bit for bit) and bias_grad[c] = sum over pixels of grad_out[p][c] from the same pass: the
//                            gradient is read once, where the mask pass followed by torch's channel sum reads it twice.
//   (c) sliced_sum_partial_kernel<L1Term> + sliced_sum_final_kernel
//                            one level of the multi-scale L1 loss: sum |out - target| / (3 n_pix) added into a device scalar, and
//                            the gradient sign(out - target) * k stored beside it.
//
// The patch map of (a): dib_deblur_patch.h.  THE SUMMATION ORDER of (b) and (c), fixed by the shape alone, and the depth of its tree:
// dib_sliced_sum.h; what is here of it is (b)'s two-dimensional geometry (bias_grad_geometry) and the terms of (c).
#include "dib_deblur_patch.h"
#include "dib_eltwise_vec.h"      // host side: misaligned, launch; F32Lane::select, F16Lane::select
#include "dib_sliced_sum.h"

namespace dib {

// ---- (a) patches -----------------------------------------------------------------------------------------------------------------
struct PatchBatch { PatchDesc d[PATCH_MAX_BATCH]; };

template <typename T>
__global__ __launch_bounds__(256) void patches_kernel(PatchBatch batch, int ps, T *__restrict__ out) {
  const PatchDesc d = batch.d[blockIdx.z];
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= (unsigned)(ps * ps)) return;
  const int c = blockIdx.y, y = (int)(e / (unsigned)ps), x = (int)(e % (unsigned)ps);
  out[((size_t)blockIdx.z * 3 + c) * ps * ps + e] = ((const T *)d.in)[patch_source(d, ps, c, y, x)];
}

// ---- (b) bias gradient -----------------------------------------------------------------------------------------------------------
constexpr int BG_THREADS = SS_THREADS, BG_PIXELS_PER_LANE = 16;

struct BiasGradGeom {
  long long npix;
  int C, V;        // channels; channels per lane (8, 4 or 1)
  int CV, QB, R;   // lane columns in all, per workgroup, pixel rows per workgroup
  int chunks, S;   // workgroups side by side, pixel slices
};

static BiasGradGeom bias_grad_geometry(long long npix, int C, int V) {
  BiasGradGeom g;
  g.npix = npix;
  g.C = C;
  g.V = V;
  g.CV = C / g.V;
  g.QB = g.CV < BG_THREADS ? g.CV : BG_THREADS;
  g.R = BG_THREADS / g.QB;
  g.chunks = (g.CV + g.QB - 1) / g.QB;
  g.S = slice_count(npix, (long long)g.R * BG_PIXELS_PER_LANE);
  return g;
}

// the V fp32 sums of a lane
template <int V> struct BgVec;
template <> struct BgVec<8> {
  typedef f32x8_t T;
  static __device__ __forceinline__ T zero() { return T{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; }
  static __device__ __forceinline__ T add(T a, const T b) { return a + b; }
  static __device__ __forceinline__ void store(float *p, const T v) {
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = v[k];
  }
};
template <> struct BgVec<4> {
  typedef float4 T;
  static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ T add(T a, const T b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; return a; }
  static __device__ __forceinline__ T select(const T u, unsigned m) { return F32Lane::select(u, m); }
  static __device__ __forceinline__ void store(float *p, const T v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
};
template <> struct BgVec<1> {
  typedef float T;
  static __device__ __forceinline__ T zero() { return 0.f; }
  static __device__ __forceinline__ T add(T a, const T b) { return a + b; }
  static __device__ __forceinline__ T select(const T u, unsigned) { return u; }      // no mask without C % 4 == 0
  static __device__ __forceinline__ void store(float *p, const T v) { p[0] = v; }
};

// What a lane loads and stores for those V channels, by the gradient's element type E: fp32 -- the sums' own vector -- or IEEE Half, V
// raw 16-bit words that `up` converts exactly; `select` moves the words and converts nothing.
template <typename E, int V> struct BgStore;
template <int V> struct BgStore<float, V> {
  typedef typename BgVec<V>::T Raw;
  static __device__ __forceinline__ Raw up(const Raw u) { return u; }
  static __device__ __forceinline__ Raw select(const Raw u, unsigned m) { return BgVec<V>::select(u, m); }
};
template <> struct BgStore<_Float16, 8> {
  typedef uint4 Raw;
  static __device__ __forceinline__ f32x8_t up(const Raw u) { return __builtin_convertvector(__builtin_bit_cast(f16x8_t, u), f32x8_t); }
  static __device__ __forceinline__ Raw select(const Raw u, unsigned m) { return F16Lane::select(u, m); }
};
template <> struct BgStore<_Float16, 1> {
  typedef unsigned short Raw;
  static __device__ __forceinline__ float up(const Raw u) { return (float)__builtin_bit_cast(_Float16, u); }
  static __device__ __forceinline__ Raw select(const Raw u, unsigned) { return u; }      // no mask without C % 8 == 0
};

// grad_in and grad_out may be the same tensor (no __restrict__): a lane reads its vector before it writes it, and no other lane
// touches that vector.
template <typename E, int V, bool MASK, bool WRITE>
__global__ __launch_bounds__(BG_THREADS) void bias_grad_partial_kernel(const typename BgStore<E, V>::Raw *grad_in, const unsigned char *__restrict__ mask,
                                                                       typename BgStore<E, V>::Raw *grad_out, BiasGradGeom g, float *__restrict__ partial) {
  typedef typename BgVec<V>::T T;
  typedef BgStore<E, V> St;
  __shared__ T sh[BG_THREADS];
  const int t = threadIdx.x;
  const int qi = t % g.QB, row = t / g.QB;
  const int q = blockIdx.y * g.QB + qi;
  const int s = blockIdx.x;
  const bool active = row < g.R && q < g.CV;
  T acc = BgVec<V>::zero();
  if (active) {
    const long long p1 = slice_begin(g.npix, g.S, s + 1);
    for (long long p = slice_begin(g.npix, g.S, s) + row; p < p1; p += g.R) {
      const long long i = p * g.CV + q;
      typename St::Raw v = grad_in[i];
      if (MASK) v = St::select(v, mask[i]);
      if (WRITE) grad_out[i] = v;
      acc = BgVec<V>::add(acc, St::up(v));
    }
  }
  sh[t] = acc;
  __syncthreads();
  row_tree<BgVec<V>>(sh, t, row, active, g.R, g.QB);
  if (active && row == 0) BgVec<V>::store(partial + (long long)s * g.C + (long long)q * V, sh[t]);
}

// The S partial sums of a channel in slice order.  A workgroup serves BG_FINAL_CH channels: all of its lanes bring the [S][4] partial
// sums into LDS at once (the partial sums were just written by workgroups on other XCDs: one memory round trip instead of S
// dependent ones -- a lane per channel walking the workspace took 42 us per call at S = 1024), then one lane per channel adds its
// row from LDS, slice 0 first.  Rows are padded by one word so that the four adding lanes read four different banks.
constexpr int BG_FINAL_CH = 4;
__global__ __launch_bounds__(BG_THREADS) void bias_grad_final_kernel(const float *__restrict__ partial, int S, int C, float *__restrict__ bias_grad) {
  __shared__ float sh[BG_FINAL_CH][SS_MAX_SLICES + 1];
  const int c0 = blockIdx.x * BG_FINAL_CH, t = threadIdx.x;
  for (int s = t; s < S; s += BG_THREADS)
#pragma unroll
    for (int k = 0; k < BG_FINAL_CH; ++k)
      if (c0 + k < C) sh[k][s] = partial[(long long)s * C + c0 + k];
  __syncthreads();
  if (t >= BG_FINAL_CH || c0 + t >= C) return;
  float acc = sh[t][0];
#pragma unroll 8
  for (int s = 1; s < S; ++s) acc += sh[t][s];
  bias_grad[c0 + t] = acc;
}

template <typename E, int V>
static int bias_grad_run(const void *grad_in, const unsigned char *mask, void *grad_out, const BiasGradGeom &g, float *bias_grad,
                         float *work, hipStream_t s) {
  typedef typename BgStore<E, V>::Raw Raw;
  const dim3 grid((unsigned)g.S, (unsigned)g.chunks);
  auto kernel = mask ? bias_grad_partial_kernel<E, V, true, true>
                     : grad_out ? bias_grad_partial_kernel<E, V, false, true> : bias_grad_partial_kernel<E, V, false, false>;
  hipLaunchKernelGGL(kernel, grid, dim3(BG_THREADS), 0, s, (const Raw *)grad_in, mask, (Raw *)grad_out, g, work);
  DIB_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(bias_grad_final_kernel, dim3((unsigned)((g.C + BG_FINAL_CH - 1) / BG_FINAL_CH)), dim3(BG_THREADS), 0, s, (const float *)work,
                     g.S, g.C, bias_grad);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

// ---- (c) L1 loss of one pyramid level -----------------------------------------------------------------------------------------
struct L1Term {
  const float *out, *target;
  int t_stride;
  float k;
  float *grad;
  // d = out - target; grad = sign(d) * k: +-k, 0 for d == 0 (either sign of zero), d itself (a NaN) when d is a NaN
  __device__ __forceinline__ float operator()(long long e) const {
    const long long p = e / 3;
    const int c = (int)(e - p * 3);
    const float d = out[e] - target[p * t_stride + c];
    grad[e] = d != d ? d : d > 0.f ? k : d < 0.f ? -k : 0.f;
    return fabsf(d);
  }
};

}  // namespace dib

using namespace dib;

extern "C" int dib_deblur_patches(const void *const *in_dev, int dtype, const int *H, const int *W, const int *py, const int *px,
                                  const unsigned int *flags, int B, int ps, void *out_dev, void *stream) {
  static const char who[] = "dib_deblur_patches";
  if (dtype != DIB_F16 && dtype != DIB_F32) { set_error("%s: unknown dtype %d", who, dtype); return DIB_EINVAL; }
  if (B < 0 || B > PATCH_MAX_BATCH || ps < 1 || ps > 32768) { set_error("%s: needs 0 <= B <= %d and 1 <= ps <= 32768", who, PATCH_MAX_BATCH); return DIB_EINVAL; }
  if (B == 0) return DIB_OK;
  if (!in_dev || !H || !W || !py || !px || !flags || !out_dev) { set_error("%s: null pointer", who); return DIB_EINVAL; }
  const size_t elem = dtype == DIB_F16 ? 2 : 4;
  if (((uintptr_t)out_dev & (elem - 1)) != 0) { set_error("%s: out_dev must be aligned to its element", who); return DIB_EINVAL; }
  PatchBatch batch;
  for (int b = 0; b < B; ++b) {
    const int code = patch_desc(who, b, in_dev[b], elem, H[b], W[b], py[b], px[b], flags[b], ps, &batch.d[b]);
    if (code != DIB_OK) return code;
  }
  const dim3 grid((unsigned)(((long long)ps * ps + 255) / 256), 3u, (unsigned)B);
  if (dtype == DIB_F16) hipLaunchKernelGGL(patches_kernel<unsigned short>, grid, dim3(256), 0, (hipStream_t)stream, batch, ps, (unsigned short *)out_dev);
  else hipLaunchKernelGGL(patches_kernel<unsigned int>, grid, dim3(256), 0, (hipStream_t)stream, batch, ps, (unsigned int *)out_dev);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

extern "C" size_t dib_bias_grad_workspace_bytes(long long n_pix, int C) {
  if (n_pix <= 0 || C <= 0) return 0;
  return (size_t)bias_grad_geometry(n_pix, C, (C % 4) == 0 ? 4 : 1).S * (size_t)C * sizeof(float);
}

// Arguments that both element types refuse alike; `lanes`: the channel multiple a mask needs
static bool bias_grad_args_ok(const char *who, const void *grad_in, const unsigned char *mask, const void *grad_out, long long n_pix, int C,
                              const float *bias_grad, const void *work, int lanes) {
  if (n_pix <= 0 || C <= 0 || n_pix > (1ll << 40) / C) { set_error("%s: needs n_pix > 0, C > 0 and n_pix * C <= 2^40", who); return false; }
  if (C > 65535 * 256) { set_error("%s: C = %d", who, C); return false; }
  if (!grad_in || !bias_grad || !work) { set_error("%s: null pointer", who); return false; }
  if (mask && !grad_out) { set_error("%s: a mask without grad_out_dev", who); return false; }
  if (mask && (C % lanes) != 0) { set_error("%s: a mask needs C %% %d == 0 (C = %d)", who, lanes, C); return false; }
  return true;
}

extern "C" int dib_bias_grad_nhwc(const float *grad_in_dev, const unsigned char *mask_dev, float *grad_out_dev, long long n_pix, int C,
                                  float *bias_grad_dev, void *work_dev, void *stream) {
  static const char who[] = "dib_bias_grad_nhwc";
  if (!bias_grad_args_ok(who, grad_in_dev, mask_dev, grad_out_dev, n_pix, C, bias_grad_dev, work_dev, 4)) return DIB_EINVAL;
  const BiasGradGeom g = bias_grad_geometry(n_pix, C, (C % 4) == 0 ? 4 : 1);
  const uintptr_t bits = (uintptr_t)grad_in_dev | (uintptr_t)grad_out_dev | (uintptr_t)bias_grad_dev | (uintptr_t)work_dev;
  if ((bits & (g.V == 4 ? 15 : 3)) != 0) { set_error("%s: tensors must be %d-byte aligned", who, g.V == 4 ? 16 : 4); return DIB_EINVAL; }
  return g.V == 4 ? bias_grad_run<float, 4>(grad_in_dev, mask_dev, grad_out_dev, g, bias_grad_dev, (float *)work_dev, (hipStream_t)stream)
                  : bias_grad_run<float, 1>(grad_in_dev, mask_dev, grad_out_dev, g, bias_grad_dev, (float *)work_dev, (hipStream_t)stream);
}

// V = 8 needs 16-byte aligned gradients; anything else takes one channel per lane.  The workspace is sized for that form, whose slices
// are the shorter ones (R is smaller), so that it serves either.
static bool bias_grad_f16_wide(const void *grad_in, const void *grad_out, int C) { return (C % 8) == 0 && !misaligned({grad_in, grad_out}); }

extern "C" size_t dib_bias_grad_f16_workspace_bytes(long long n_pix, int C) {
  if (n_pix <= 0 || C <= 0) return 0;
  return (size_t)bias_grad_geometry(n_pix, C, 1).S * (size_t)C * sizeof(float);
}

extern "C" int dib_bias_grad_f16_nhwc(const void *grad_in_dev, const unsigned char *mask_dev, void *grad_out_dev, long long n_pix, int C,
                                      float *bias_grad_dev, void *work_dev, void *stream) {
  static const char who[] = "dib_bias_grad_f16_nhwc";
  if (!bias_grad_args_ok(who, grad_in_dev, mask_dev, grad_out_dev, n_pix, C, bias_grad_dev, work_dev, 8)) return DIB_EINVAL;
  if ((((uintptr_t)grad_in_dev | (uintptr_t)grad_out_dev) & 1) != 0 || (((uintptr_t)bias_grad_dev | (uintptr_t)work_dev) & 3) != 0) {
    set_error("%s: tensors must be aligned to their elements", who);
    return DIB_EINVAL;
  }
  const bool wide = bias_grad_f16_wide(grad_in_dev, grad_out_dev, C);
  if (mask_dev && !wide) { set_error("%s: with a mask the gradients must be 16-byte aligned", who); return DIB_EINVAL; }
  const BiasGradGeom g = bias_grad_geometry(n_pix, C, wide ? 8 : 1);
  return wide ? bias_grad_run<_Float16, 8>(grad_in_dev, mask_dev, grad_out_dev, g, bias_grad_dev, (float *)work_dev, (hipStream_t)stream)
              : bias_grad_run<_Float16, 1>(grad_in_dev, mask_dev, grad_out_dev, g, bias_grad_dev, (float *)work_dev, (hipStream_t)stream);
}

extern "C" size_t dib_l1_pyramid_loss_workspace_bytes(long long n_pix) {
  if (n_pix <= 0) return 0;
  return (size_t)scalar_slices(3 * n_pix) * sizeof(float);
}

extern "C" int dib_l1_pyramid_loss(const float *out_dev, const float *target_dev, int target_stride, long long n_pix, float gscale,
                                   float *grad_dev, float *loss_dev, void *work_dev, void *stream) {
  static const char who[] = "dib_l1_pyramid_loss";
  if (n_pix <= 0 || n_pix > (1ll << 38)) { set_error("%s: needs 0 < n_pix <= 2^38", who); return DIB_EINVAL; }
  if (target_stride < 3) { set_error("%s: target_stride %d (channels 0..2 of each pixel are read)", who, target_stride); return DIB_EINVAL; }
  if (!out_dev || !target_dev || !grad_dev || !loss_dev || !work_dev) { set_error("%s: null pointer", who); return DIB_EINVAL; }
  const uintptr_t bits = (uintptr_t)out_dev | (uintptr_t)target_dev | (uintptr_t)grad_dev | (uintptr_t)loss_dev | (uintptr_t)work_dev;
  if ((bits & 3) != 0) { set_error("%s: tensors must be 4-byte aligned", who); return DIB_EINVAL; }
  const long long n = 3 * n_pix;
  return sliced_sum_run(L1Term{out_dev, target_dev, target_stride, gscale / (float)n, grad_dev}, n, loss_dev, (float *)work_dev, (hipStream_t)stream);
}
