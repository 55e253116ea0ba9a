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
//   (c) l1_partial_kernel + l1_final_kernel
//                            one level of the multi-scale L1 loss: sum |out - target| / (3 n_pix) added into a device scalar, and
//                            the gradient sign(out - target) * k stored beside it.
//
// THE SUMMATION ORDER of (b) and (c) is fixed by the shape alone, so two calls on the same input agree bit for bit:
//   (b) the [n_pix][C] gradient is cut into S slices of consecutive pixels (bias_grad_geometry below: S = ceil(n_pix / (16 R))
//       capped at 1024).  A workgroup of 256 lanes takes one slice and QB = min(C / V, 256) lane columns (V = 4 channels per lane
//       when C % 4 == 0, else 1; the Half form, dib_bias_grad_f16_nhwc: V = 8 when C % 8 == 0 and the gradient is 16-byte aligned,
//       else 1 -- one 16-byte load per lane either way, and every Half is exact in fp32, so only the additions below round); lane
//       (row, column) adds the pixels slice_begin + row, + R, + 2 R, ... (R = 256 / QB) one after the other: a chain of at most L = ceil(slice length / R) additions.  The R rows are then added in LDS as a tree (row r takes row
//       r + h for h = the powers of two below R, largest first): ceil(log2 R) levels.  The slice's partial sums go to the workspace
//       [S][C]; the second launch adds them for each channel in slice order, starting from slice 0: S - 1 additions.
//       DEPTH of the tree, the number of fp32 additions any one input can pass through:  L + ceil(log2 R) + S - 1.
//       Every addition rounds once, so |bias_grad - exact| <= depth * 2^-24 * sum |grad_out| (first order in 2^-24).
//   (c) the 3 n_pix differences, in memory order, are cut into S = ceil(3 n_pix / 2048) (capped at 1024) slices; lane t of a
//       slice's workgroup adds |d| of elements slice_begin + t, + 256, ...: a chain of L = ceil(slice length / 256); the 256 lanes
//       are added as a tree of 8 levels; the second launch adds the S partial sums in slice order, divides by float(3 n_pix) and adds
//       the result to the loss scalar.  DEPTH = L + 8 + S - 1 additions, then one division and one addition onto the scalar.
// models/deblur_train.py restates both geometries (bias_grad_depth, l1_loss_depth) for the tests' error bounds.  The order itself is
// restated in numpy float32 from this comment (tests/test_deblur_train.py: restated_bias_grad, restated_l1), and
// tests/test_deblur_train_geometry_gpu.py holds the kernels to it bit for bit at S = 1024: change the order here and there together.
#include "dib_eltwise_vec.h"      // host side: misaligned, launch; F32Lane::select, F16Lane::select

namespace dib {

// ---- (a) patches -----------------------------------------------------------------------------------------------------------------
constexpr int PATCH_MAX_BATCH = 64;
struct PatchDesc {
  const void *in;      // planar [3][H][W]
  int H, W, py, px;
  unsigned flags;      // DIB_PATCH_HFLIP | DIB_PATCH_VFLIP | DIB_PATCH_ROT90 | channel order in bits 4..9
  int pad_;
};
struct PatchBatch { PatchDesc d[PATCH_MAX_BATCH]; };

// out[b][c][y][x] = in_b[order[c]][py + y1][px + x0]: dataCommon.py's order -- crop, hflip (reverse x), vflip (reverse y), rot90
// (transpose), channel order -- read backwards from the output element.
template <typename T>
__global__ __launch_bounds__(256) void patches_kernel(PatchBatch batch, int ps, T *__restrict__ out) {
  const PatchDesc d = batch.d[blockIdx.z];
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= (unsigned)(ps * ps)) return;
  const int c = blockIdx.y, y = (int)(e / (unsigned)ps), x = (int)(e % (unsigned)ps);
  const bool rot = d.flags & DIB_PATCH_ROT90;
  const int y2 = rot ? x : y, x2 = rot ? y : x;
  const int y1 = (d.flags & DIB_PATCH_VFLIP) ? ps - 1 - y2 : y2;
  const int x0 = (d.flags & DIB_PATCH_HFLIP) ? ps - 1 - x2 : x2;
  const int cs = (int)((d.flags >> (4 + 2 * c)) & 3u);
  const T *src = (const T *)d.in;
  out[((size_t)blockIdx.z * 3 + c) * ps * ps + e] = src[((size_t)cs * d.H + (d.py + y1)) * d.W + (d.px + x0)];
}

// ---- (b) bias gradient -----------------------------------------------------------------------------------------------------------
constexpr int BG_THREADS = 256, BG_MAX_SLICES = 1024, BG_PIXELS_PER_LANE = 16;

struct BiasGradGeom {
  long long npix;
  int C, V;        // channels; channels per lane (8, 4 or 1)
  int CV, QB, R;   // lane columns in all, per workgroup, pixel rows per workgroup
  int chunks, S;   // workgroups side by side, pixel slices
};

__host__ __device__ inline long long bg_slice_begin(long long n, int S, int s) { return n / S * s + (n % S < s ? n % S : s); }

static BiasGradGeom bias_grad_geometry(long long npix, int C, int V) {
  BiasGradGeom g;
  g.npix = npix;
  g.C = C;
  g.V = V;
  g.CV = C / g.V;
  g.QB = g.CV < BG_THREADS ? g.CV : BG_THREADS;
  g.R = BG_THREADS / g.QB;
  g.chunks = (g.CV + g.QB - 1) / g.QB;
  const long long per = (long long)g.R * BG_PIXELS_PER_LANE;
  long long S = (npix + per - 1) / per;
  if (S > BG_MAX_SLICES) S = BG_MAX_SLICES;
  if (S < 1) S = 1;
  g.S = (int)S;
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
    const long long p1 = bg_slice_begin(g.npix, g.S, s + 1);
    for (long long p = bg_slice_begin(g.npix, g.S, s) + row; p < p1; p += g.R) {
      const long long i = p * g.CV + q;
      typename St::Raw v = grad_in[i];
      if (MASK) v = St::select(v, mask[i]);
      if (WRITE) grad_out[i] = v;
      acc = BgVec<V>::add(acc, St::up(v));
    }
  }
  sh[t] = acc;
  __syncthreads();
  int h = 1;
  while (h < g.R) h <<= 1;
  for (h >>= 1; h >= 1; h >>= 1) {
    if (active && row < h && row + h < g.R) sh[t] = BgVec<V>::add(sh[t], sh[t + h * g.QB]);
    __syncthreads();
  }
  if (active && row == 0) BgVec<V>::store(partial + (long long)s * g.C + (long long)q * V, sh[t]);
}

// The S partial sums of a channel in slice order.  A workgroup serves BG_FINAL_CH channels: all of its lanes bring the [S][4] partial
// sums into LDS at once (the partial sums were just written by workgroups on other XCDs: one memory round trip instead of S
// dependent ones -- a lane per channel walking the workspace took 42 us per call at S = 1024), then one lane per channel adds its
// row from LDS, slice 0 first.  Rows are padded by one word so that the four adding lanes read four different banks.
constexpr int BG_FINAL_CH = 4;
__global__ __launch_bounds__(BG_THREADS) void bias_grad_final_kernel(const float *__restrict__ partial, int S, int C, float *__restrict__ bias_grad) {
  __shared__ float sh[BG_FINAL_CH][BG_MAX_SLICES + 1];
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
constexpr int L1_THREADS = 256, L1_MAX_SLICES = 1024, L1_ELEMS_PER_LANE = 8;

static int l1_slices(long long n_elems) {
  const long long per = (long long)L1_THREADS * L1_ELEMS_PER_LANE;
  long long S = (n_elems + per - 1) / per;
  if (S > L1_MAX_SLICES) S = L1_MAX_SLICES;
  return S < 1 ? 1 : (int)S;
}

// d = out - target; grad = sign(d) * k: +-k, 0 for d == 0 (either sign of zero), d itself (a NaN) when d is a NaN
__global__ __launch_bounds__(L1_THREADS) void l1_partial_kernel(const float *__restrict__ out, const float *__restrict__ target, int t_stride,
                                                                long long n_elems, int S, float k, float *__restrict__ grad,
                                                                float *__restrict__ partial) {
  __shared__ float sh[L1_THREADS];
  const int t = threadIdx.x, s = blockIdx.x;
  const long long e1 = bg_slice_begin(n_elems, S, s + 1);
  float acc = 0.f;
  for (long long e = bg_slice_begin(n_elems, S, s) + t; e < e1; e += L1_THREADS) {
    const long long p = e / 3;
    const int c = (int)(e - p * 3);
    const float d = out[e] - target[p * t_stride + c];
    grad[e] = d != d ? d : d > 0.f ? k : d < 0.f ? -k : 0.f;
    acc += fabsf(d);
  }
  sh[t] = acc;
  __syncthreads();
  for (int h = L1_THREADS / 2; h >= 1; h >>= 1) {
    if (t < h) sh[t] += sh[t + h];
    __syncthreads();
  }
  if (t == 0) partial[s] = sh[0];
}

__global__ void l1_final_kernel(const float *__restrict__ partial, int S, float n, float *loss) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float acc = partial[0];
  for (int s = 1; s < S; ++s) acc += partial[s];
  *loss = *loss + acc / n;
}

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
    if (!in_dev[b] || ((uintptr_t)in_dev[b] & (elem - 1)) != 0) { set_error("%s: image %d: null or misaligned pointer", who, b); return DIB_EINVAL; }
    if (H[b] < ps || W[b] < ps || py[b] < 0 || px[b] < 0 || py[b] > H[b] - ps || px[b] > W[b] - ps) {
      set_error("%s: image %d: a %d x %d patch at (%d, %d) leaves the %d x %d image", who, b, ps, ps, py[b], px[b], H[b], W[b]);
      return DIB_ESHAPE;
    }
    const unsigned f = flags[b];
    if ((f & ~(7u | (63u << 4))) != 0 || ((f >> 4) & 3u) == 3u || ((f >> 6) & 3u) == 3u || ((f >> 8) & 3u) == 3u) {
      set_error("%s: image %d: flags 0x%x (three flip bits, three channel indices 0..2 in bits 4..9)", who, b, f);
      return DIB_EINVAL;
    }
    batch.d[b] = {in_dev[b], H[b], W[b], py[b], px[b], f, 0};
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
  return (size_t)l1_slices(3 * n_pix) * sizeof(float);
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
  const int S = l1_slices(n);
  const float denom = (float)n;
  hipLaunchKernelGGL(l1_partial_kernel, dim3((unsigned)S), dim3(L1_THREADS), 0, (hipStream_t)stream, out_dev, target_dev, target_stride, n, S,
                     gscale / denom, grad_dev, (float *)work_dev);
  DIB_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float *)work_dev, S, denom, loss_dev);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}
