// The deblur-first stage (reference engine.py:319-322 around models/deblur/deblurInterface.py:42-63): everything of it that is not a
// convolution.  The reference sends the image to the host as 8-bit, pads it with numpy, builds a Gaussian pyramid with scikit-image,
// uploads three levels, runs MSResNet, fixes the result up and uploads it again; here the image never leaves the device:
//   dib_deblur_pyramid         quantise to 8 bits, edge-pad, Gaussian pyramid, mean shift -> the network's channels-last inputs
//   dib_deblur_shuffle_concat  conv_end's bias + PixelShuffle(2) into channels 3..5 of the next finer level's input (no cat)
//   dib_deblur_finish          last bias, mean shift back, + 0.5, clamp, / 255, crop -> the planar fp32 image the detector gets
// All three are memory-bound streams: one pass, vector loads and stores where the sizes allow, no scratch.  Values: include/dib.h.
// Each has a Half form (dib_deblur_*_f16, `--deblur_precision half`): the same kernels templated over the stored type, every value
// rounded to Half (to nearest even) where the reference's Half tensors round it.
#include <hip/hip_fp16.h>
#include <math.h>

#include "dib_common.h"

namespace dib {

constexpr int DBL_LANES = 256, DBL_PIX = 4;
constexpr int DBL_RADIUS = 3;                                  // int(4 * sigma + 0.5) at sigma = 2 / 3
constexpr int DBL_TILE = 16, DBL_SRC = 2 * DBL_TILE;           // output pixels per workgroup side, source pixels under them
constexpr int DBL_WIN = DBL_SRC + 2 * DBL_RADIUS;              // ... with the halo: 38
constexpr float DBL_MEAN = 127.5f;                             // rgb_range / 2
constexpr long long DBL_MAX_PIXELS = 1ll << 30;

struct GaussTaps { float w[DBL_RADIUS + 1]; };                 // w[|d|], normalised over the 7 taps

// scipy.ndimage's "reflect" (d c b a | a b c d), periodic: any integer -> [0, n)
__device__ __forceinline__ int reflect_index(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// step 1 of the stage: (x * 255) in the image's own dtype, truncated towards zero, clamped to 0..255 (NaN -> 0)
__device__ __forceinline__ float quantise(float x, bool is_half) {
  float a = x * 255.0f;
  if (is_half) a = __half2float(__float2half(a));              // the Half product is rounded to Half before the truncation
  return a >= 255.0f ? 255.0f : (a > 0.0f ? truncf(a) : 0.0f);
}

__device__ __forceinline__ float to_float(__half v) { return __half2float(v); }
__device__ __forceinline__ float to_float(float v) { return v; }

__device__ __forceinline__ void ld4(const __half *p, float v[4]) {
  const uint2 w = *reinterpret_cast<const uint2 *>(p);
  v[0] = __half2float(__ushort_as_half((unsigned short)(w.x & 0xffffu)));
  v[1] = __half2float(__ushort_as_half((unsigned short)(w.x >> 16)));
  v[2] = __half2float(__ushort_as_half((unsigned short)(w.y & 0xffffu)));
  v[3] = __half2float(__ushort_as_half((unsigned short)(w.y >> 16)));
}
__device__ __forceinline__ void ld4(const float *p, float v[4]) {
  const float4 w = *reinterpret_cast<const float4 *>(p);
  v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
}

// ---- the Half forms: what is stored is rounded to nearest even (v_cvt_f16_f32), one rounding per op of the reference's Half graph ----
__device__ __forceinline__ float round_half(float v) { return __half2float(__float2half(v)); }
__device__ __forceinline__ unsigned short half_bits(float v) { return __half_as_ushort(__float2half(v)); }
__device__ __forceinline__ unsigned pack_half2(float a, float b) { return (unsigned)half_bits(a) | ((unsigned)half_bits(b) << 16); }
__device__ __forceinline__ float half_lo(unsigned u) { return __half2float(__ushort_as_half((unsigned short)(u & 0xffffu))); }
__device__ __forceinline__ float half_hi(unsigned u) { return __half2float(__ushort_as_half((unsigned short)(u >> 16))); }
// a level's element from the fp32 value L of the 0..255 pyramid: fp32 levels hold L - 127.5; Half levels hold what MSResNet's Half
// `x - 127.5` makes of the Half tensor the reference uploads: half(half(L) - 127.5)
__device__ __forceinline__ float level_value(float L, float *) { return L - DBL_MEAN; }
__device__ __forceinline__ float level_value(float L, __half *) { return round_half(L) - DBL_MEAN; }
__device__ __forceinline__ void st1(float *p, float v) { *p = v; }
__device__ __forceinline__ void st1(__half *p, float v) { *p = __float2half(v); }

// Level 0: quantise, edge-pad and convert in one pass.  A lane owns four consecutive pixels of one padded row.
// in: planar [3][H][W]; out: [Hp][Wp][cs] (cs = 3 or 6), channels 0..2 written.  vec bit 0: the planes take 4-element loads (W % 4 == 0,
// aligned); bit 1: a 3-channel output row takes 16-byte stores (Wp % 4 == 0).
// O = __half: the same records at half the size (a 3-channel row of four pixels is three 8-byte stores, a 6-channel pixel 4 + 2 bytes).
template <typename T, typename O>
__global__ __launch_bounds__(DBL_LANES) void deblur_level0_kernel(const T *__restrict__ in, O *__restrict__ out, int H, int W, int Hp,
                                                                  int Wp, int cs, int vec) {
  constexpr bool half_out = sizeof(O) == 2;
  constexpr bool is_half = sizeof(T) == 2;
  const int per_row = (Wp + DBL_PIX - 1) / DBL_PIX;
  const int g = blockIdx.x * DBL_LANES + threadIdx.x;
  if (g >= Hp * per_row) return;
  const int y = g / per_row, x0 = (g - y * per_row) * DBL_PIX;
  const int count = min(DBL_PIX, Wp - x0);
  const int sy = min(y, H - 1);
  const size_t plane = (size_t)H * W;
  const T *row = in + (size_t)sy * W;
  float q[3][DBL_PIX];
  if ((vec & 1) && x0 + DBL_PIX <= W) {
#pragma unroll
    for (int c = 0; c < 3; ++c) ld4(row + c * plane + x0, q[c]);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < DBL_PIX; ++k) q[c][k] = to_float(row[c * plane + min(x0 + k, W - 1)]);      // edge padding on the right
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < DBL_PIX; ++k) q[c][k] = quantise(q[c][k], is_half) - DBL_MEAN;      // a multiple of 0.5 below 128: exact in Half too
  O *o = out + ((size_t)y * Wp + x0) * cs;
  if constexpr (half_out) {
    if (cs == 3 && (vec & 2) && count == DBL_PIX) {                    // 12 consecutive Half on an 8-byte boundary
      uint2 *o2 = reinterpret_cast<uint2 *>(o);
      o2[0] = make_uint2(pack_half2(q[0][0], q[1][0]), pack_half2(q[2][0], q[0][1]));
      o2[1] = make_uint2(pack_half2(q[1][1], q[2][1]), pack_half2(q[0][2], q[1][2]));
      o2[2] = make_uint2(pack_half2(q[2][2], q[0][3]), pack_half2(q[1][3], q[2][3]));
    } else if (cs == 6) {                                              // 12-byte records: 4 bytes + 2 bytes each
#pragma unroll
      for (int k = 0; k < DBL_PIX; ++k) {
        if (k < count) {
          *reinterpret_cast<unsigned *>(o + 6 * k) = pack_half2(q[0][k], q[1][k]);
          st1(o + 6 * k + 2, q[2][k]);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < DBL_PIX; ++k) {
        if (k < count) { st1(o + 3 * k, q[0][k]); st1(o + 3 * k + 1, q[1][k]); st1(o + 3 * k + 2, q[2][k]); }
      }
    }
  } else {
    if (cs == 3 && (vec & 2) && count == DBL_PIX) {                    // 12 consecutive floats on a 16-byte boundary
      float4 *o4 = reinterpret_cast<float4 *>(o);
      o4[0] = make_float4(q[0][0], q[1][0], q[2][0], q[0][1]);
      o4[1] = make_float4(q[1][1], q[2][1], q[0][2], q[1][2]);
      o4[2] = make_float4(q[2][2], q[0][3], q[1][3], q[2][3]);
    } else if (cs == 6) {                                              // 24-byte records: 8 bytes + 4 bytes each
#pragma unroll
      for (int k = 0; k < DBL_PIX; ++k) {
        if (k < count) {
          *reinterpret_cast<float2 *>(o + 6 * k) = make_float2(q[0][k], q[1][k]);
          o[6 * k + 2] = q[2][k];
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < DBL_PIX; ++k) {
        if (k < count) { o[3 * k] = q[0][k]; o[3 * k + 1] = q[1][k]; o[3 * k + 2] = q[2][k]; }
      }
    }
  }
}

// One tap loop of the separable filter: the seven products are accumulated from the first tap to the last, each step rounded
__device__ __forceinline__ float gauss7(const float *p, int stride, const GaussTaps &g) {
  float acc = g.w[3] * p[0];
#pragma unroll
  for (int k = 1; k <= 2 * DBL_RADIUS; ++k) acc = acc + g.w[k < DBL_RADIUS ? DBL_RADIUS - k : k - DBL_RADIUS] * p[k * stride];
  return acc;
}

// Level s >= 1 from level s - 1 (h x w, both even): smooth down the columns (axis 0), then along the rows (axis 1), mean of each 2 x 2
// block.  A workgroup makes 16 x 16 output pixels from a 38 x 38 source window in LDS (the 3-pixel halo reflected, periodically: a
// 2 x 2 level is legal).  Levels are stored minus 127.5; the filter runs on the 0..255 values.
// Half levels (O = __half): the pyramid itself stays fp32, as the reference builds it on the host, and only what is stored is rounded.
// A Half level 0 is exact (I = __half reads it); a coarser Half level is not, so the next one is filtered from the fp32 copy that
// SIDE leaves in `side` ([h / 2][w / 2][3], minus 127.5 like an fp32 level; I = float reads it with cs_in = 3).
template <typename I, typename O, bool SIDE>
__global__ __launch_bounds__(DBL_LANES) void deblur_down_kernel(const I *__restrict__ in, O *__restrict__ out, float *__restrict__ side,
                                                                int h, int w, int cs_in, int cs_out, const GaussTaps g) {
  __shared__ float s_in[3][DBL_WIN][DBL_WIN + 1];
  __shared__ float s_col[3][DBL_SRC][DBL_WIN + 1];
  const int tid = threadIdx.x;
  const int oy0 = blockIdx.y * DBL_TILE, ox0 = blockIdx.x * DBL_TILE;
  const int iy0 = 2 * oy0 - DBL_RADIUS, ix0 = 2 * ox0 - DBL_RADIUS;
  for (int i = tid; i < DBL_WIN * DBL_WIN; i += DBL_LANES) {
    const int r = i / DBL_WIN, c = i - r * DBL_WIN;
    const I *p = in + ((size_t)reflect_index(iy0 + r, h) * w + reflect_index(ix0 + c, w)) * cs_in;
    s_in[0][r][c] = to_float(p[0]) + DBL_MEAN;
    s_in[1][r][c] = to_float(p[1]) + DBL_MEAN;
    s_in[2][r][c] = to_float(p[2]) + DBL_MEAN;
  }
  __syncthreads();
  for (int i = tid; i < DBL_SRC * DBL_WIN; i += DBL_LANES) {
    const int r = i / DBL_WIN, c = i - r * DBL_WIN;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) s_col[ch][r][c] = gauss7(&s_in[ch][r][c], DBL_WIN + 1, g);
  }
  __syncthreads();
  const int ty = tid / DBL_TILE, tx = tid - ty * DBL_TILE;
  const int oy = oy0 + ty, ox = ox0 + tx;
  if (oy >= h / 2 || ox >= w / 2) return;
  float m[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float a = gauss7(&s_col[ch][2 * ty][2 * tx], 1, g), b = gauss7(&s_col[ch][2 * ty][2 * tx + 1], 1, g);
    const float c = gauss7(&s_col[ch][2 * ty + 1][2 * tx], 1, g), d = gauss7(&s_col[ch][2 * ty + 1][2 * tx + 1], 1, g);
    m[ch] = 0.25f * ((a + b) + (c + d));
  }
  const size_t pixel = (size_t)oy * (w / 2) + ox;
  O *o = out + pixel * cs_out;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) st1(o + ch, level_value(m[ch], o));
  if (SIDE) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) side[pixel * 3 + ch] = m[ch] - DBL_MEAN;
  }
}

// in [h][w][12] (conv_end's raw output), out [2h][2w][6]: out[2y + i][2x + j][3 + c] = in[y][x][4c + 2i + j] + bias[4c + 2i + j].
// A lane owns one source pixel: three 16-byte loads, four 12-byte records (4 + 8 bytes: a record starts 12 bytes into a 24-byte pixel).
// T = __half: three 8-byte loads (a 24-byte pixel), the sum rounded to Half, four 6-byte records (2 + 4 bytes, 6 bytes into a 12-byte pixel).
template <typename T>
__global__ __launch_bounds__(DBL_LANES) void deblur_shuffle_concat_kernel(const T *__restrict__ in, const float *__restrict__ bias,
                                                                          T *__restrict__ out, int h, int w) {
  const int i = blockIdx.x * DBL_LANES + threadIdx.x;
  if (i >= h * w) return;
  const int y = i / w, x = i - y * w;
  float v[12];
  if constexpr (sizeof(T) == 2) {
    const uint2 *p = reinterpret_cast<const uint2 *>(in) + (size_t)3 * i;
    const uint2 a = p[0], b = p[1], c = p[2];
    const unsigned u[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
#pragma unroll
    for (int k = 0; k < 6; ++k) { v[2 * k] = half_lo(u[k]) + bias[2 * k]; v[2 * k + 1] = half_hi(u[k]) + bias[2 * k + 1]; }
  } else {
    const float4 *p = reinterpret_cast<const float4 *>(in) + (size_t)3 * i;
    const float4 a = p[0], b = p[1], c = p[2];
    const float r[12] = {a.x + bias[0], a.y + bias[1], a.z + bias[2],  a.w + bias[3], b.x + bias[4],  b.y + bias[5],
                         b.z + bias[6], b.w + bias[7], c.x + bias[8],  c.y + bias[9], c.z + bias[10], c.w + bias[11]};
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = r[k];
  }
#pragma unroll
  for (int ii = 0; ii < 2; ++ii)
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      T *o = out + ((size_t)(2 * y + ii) * (2 * w) + (2 * x + jj)) * 6 + 3;
      st1(o, v[2 * ii + jj]);
      if constexpr (sizeof(T) == 2) *reinterpret_cast<unsigned *>(o + 1) = pack_half2(v[4 + 2 * ii + jj], v[8 + 2 * ii + jj]);
      else *reinterpret_cast<float2 *>(o + 1) = make_float2(v[4 + 2 * ii + jj], v[8 + 2 * ii + jj]);
    }
}

// ((v + bias) + 127.5 + 0.5) clamped to [0, 255] (a NaN stays a NaN, as torch's clamp leaves it), / 255: every step rounded on its own.
// The division is what ATen runs for `tensor / 255` on a GPU, where the reference runs it: a multiplication by the fp32 reciprocal
// (its CPU kernel divides; the two differ by at most one unit in the last place).
__device__ __forceinline__ float finish_value(float v, float b, float *) {
  float t = v + b;
  t = t + DBL_MEAN;
  t = t + 0.5f;
  t = t != t ? t : fminf(fmaxf(t, 0.0f), 255.0f);
  return t * (1.0f / 255.0f);
}
// On Half tensors every one of those ops rounds to Half; ATen forms the last product in fp32 and rounds it once (the store does)
__device__ __forceinline__ float finish_value(float v, float b, __half *) {
  float t = round_half(v + b);
  t = round_half(t + DBL_MEAN);
  t = round_half(t + 0.5f);
  t = t != t ? t : fminf(fmaxf(t, 0.0f), 255.0f);
  return t * (1.0f / 255.0f);
}

// in [Hp][Wp][3] (the finest level's last convolution, raw), out planar [3][H][W]: the crop.  A lane owns four consecutive pixels of
// one output row.  vec bit 0: 16-byte loads (Wp % 4 == 0); bit 1: 16-byte stores (W % 4 == 0).  T = __half: 8-byte loads and stores.
template <typename T>
__global__ __launch_bounds__(DBL_LANES) void deblur_finish_kernel(const T *__restrict__ in, const float *__restrict__ bias,
                                                                  T *__restrict__ out, int H, int W, int Wp, int vec) {
  const int per_row = (W + DBL_PIX - 1) / DBL_PIX;
  const int g = blockIdx.x * DBL_LANES + threadIdx.x;
  if (g >= H * per_row) return;
  const int y = g / per_row, x0 = (g - y * per_row) * DBL_PIX;
  const int count = min(DBL_PIX, W - x0);
  const T *p = in + ((size_t)y * Wp + x0) * 3;
  float v[3 * DBL_PIX];
  if ((vec & 1) && count == DBL_PIX) {
    if constexpr (sizeof(T) == 2) {
      const uint2 *p2 = reinterpret_cast<const uint2 *>(p);
      const uint2 a = p2[0], b = p2[1], c = p2[2];
      const unsigned u[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
#pragma unroll
      for (int k = 0; k < 6; ++k) { v[2 * k] = half_lo(u[k]); v[2 * k + 1] = half_hi(u[k]); }
    } else {
      const float4 *p4 = reinterpret_cast<const float4 *>(p);
      const float4 a = p4[0], b = p4[1], c = p4[2];
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 3 * DBL_PIX; ++k) v[k] = k < 3 * count ? to_float(p[k]) : 0.0f;
  }
  const size_t plane = (size_t)H * W;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float bc = bias[c];
    float r[DBL_PIX];
#pragma unroll
    for (int k = 0; k < DBL_PIX; ++k) r[k] = finish_value(v[3 * k + c], bc, (T *)nullptr);
    T *o = out + c * plane + (size_t)y * W + x0;
    if ((vec & 2) && count == DBL_PIX) {
      if constexpr (sizeof(T) == 2) *reinterpret_cast<uint2 *>(o) = make_uint2(pack_half2(r[0], r[1]), pack_half2(r[2], r[3]));
      else *reinterpret_cast<float4 *>(o) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
      for (int k = 0; k < DBL_PIX; ++k)
        if (k < count) st1(o + k, r[k]);
    }
  }
}

static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
static inline unsigned blocks_for(long long lanes) { return (unsigned)((lanes + DBL_LANES - 1) / DBL_LANES); }

// O: the levels' stored type.  work: the Half form's fp32 copies of levels 1 .. n - 2 (the sources of levels 2 .. n - 1), back to back.
template <typename O>
static int pyramid(const char *who, const void *in_dev, int dtype, int H, int W, int n_scales, O *const *levels_dev, float *work, void *stream) {
  constexpr bool half_out = sizeof(O) == 2;
  if (!in_dev || !levels_dev) { set_error("%s: null pointer", who); return DIB_EINVAL; }
  if (dtype != DIB_F16 && dtype != DIB_F32) { set_error("%s: unsupported dtype %d", who, dtype); return DIB_EINVAL; }
  if (H < 1 || W < 1) { set_error("%s: needs H, W >= 1 (got %d x %d)", who, H, W); return DIB_EINVAL; }
  if (n_scales < 1 || n_scales > 4) { set_error("%s: n_scales = %d outside 1..4", who, n_scales); return DIB_EINVAL; }
  const int div = 1 << (n_scales - 1);
  const long long Hp = ((long long)H + div - 1) / div * div, Wp = ((long long)W + div - 1) / div * div;
  if (Hp * Wp > DBL_MAX_PIXELS) { set_error("%s: the padded image has %lld pixels, more than 2^30", who, Hp * Wp); return DIB_EINVAL; }
  for (int s = 0; s < n_scales; ++s) {
    if (!levels_dev[s]) { set_error("%s: null pointer (level %d)", who, s); return DIB_EINVAL; }
    if (!aligned16(levels_dev[s])) { set_error("%s: level %d is not 16-byte aligned", who, s); return DIB_EINVAL; }
  }
  if (half_out && n_scales > 2) {
    if (!work) { set_error("%s: null pointer (workspace, needed for n_scales > 2)", who); return DIB_EINVAL; }
    if (!aligned16(work)) { set_error("%s: the workspace is not 16-byte aligned", who); return DIB_EINVAL; }
  }
  const size_t elem = dtype == DIB_F16 ? 2 : 4;
  if ((uintptr_t)in_dev % elem) { set_error("%s: the image is not aligned to its element size", who); return DIB_EINVAL; }
  const hipStream_t st = (hipStream_t)stream;
  const int cs0 = n_scales > 1 ? 6 : 3;
  const int vec = ((W % DBL_PIX) == 0 && ((uintptr_t)in_dev % (DBL_PIX * elem)) == 0 ? 1 : 0) | ((Wp % DBL_PIX) == 0 ? 2 : 0);
  const unsigned blocks = blocks_for(Hp * ((Wp + DBL_PIX - 1) / DBL_PIX));
  if (dtype == DIB_F16)
    hipLaunchKernelGGL((deblur_level0_kernel<__half, O>), dim3(blocks), dim3(DBL_LANES), 0, st, (const __half *)in_dev, levels_dev[0], H, W,
                       (int)Hp, (int)Wp, cs0, vec);
  else
    hipLaunchKernelGGL((deblur_level0_kernel<float, O>), dim3(blocks), dim3(DBL_LANES), 0, st, (const float *)in_dev, levels_dev[0], H, W,
                       (int)Hp, (int)Wp, cs0, vec);
  DIB_HIP_CHECK(hipGetLastError());
  // scipy.ndimage.gaussian_filter1d's weights at sigma = 2 / 3, truncate = 4: exp(-x^2 / (2 sigma^2)) over x = -3..3, normalised (float64)
  GaussTaps g;
  {
    const double sigma = 2.0 / 3.0;
    double w[DBL_RADIUS + 1], sum = 0.0;
    for (int d = 0; d <= DBL_RADIUS; ++d) w[d] = exp(-0.5 / (sigma * sigma) * (double)(d * d));
    for (int x = -DBL_RADIUS; x <= DBL_RADIUS; ++x) sum += w[x < 0 ? -x : x];
    for (int d = 0; d <= DBL_RADIUS; ++d) g.w[d] = (float)(w[d] / sum);
  }
  const float *src32 = nullptr;                                        // the Half form: the fp32 copy of level s - 1, s >= 2
  for (int s = 1; s < n_scales; ++s) {
    const int h = (int)(Hp >> (s - 1)), w = (int)(Wp >> (s - 1));      // the source level: both even
    const dim3 grid((unsigned)((w / 2 + DBL_TILE - 1) / DBL_TILE), (unsigned)((h / 2 + DBL_TILE - 1) / DBL_TILE));
    const int cs_out = s < n_scales - 1 ? 6 : 3;
    if constexpr (half_out) {
      const bool side = s < n_scales - 1;                              // a level that has a coarser one leaves its fp32 copy
      if (s == 1)
        hipLaunchKernelGGL((side ? deblur_down_kernel<__half, __half, true> : deblur_down_kernel<__half, __half, false>), grid, dim3(DBL_LANES),
                           0, st, (const __half *)levels_dev[0], levels_dev[1], work, h, w, 6, cs_out, g);
      else
        hipLaunchKernelGGL((side ? deblur_down_kernel<float, __half, true> : deblur_down_kernel<float, __half, false>), grid, dim3(DBL_LANES),
                           0, st, src32, levels_dev[s], work, h, w, 3, cs_out, g);
      src32 = work;
      if (side) work += (size_t)(h / 2) * (w / 2) * 3;                  // h, w multiples of 4 here: the next copy stays 16-byte aligned
    } else {
      hipLaunchKernelGGL((deblur_down_kernel<float, float, false>), grid, dim3(DBL_LANES), 0, st, (const float *)levels_dev[s - 1], levels_dev[s],
                         (float *)nullptr, h, w, 6, cs_out, g);
    }
    DIB_HIP_CHECK(hipGetLastError());
  }
  return DIB_OK;
}

template <typename T>
static int shuffle_concat(const char *who, const T *in_dev, const float *bias_dev, T *out_dev, int h, int w, void *stream) {
  if (!in_dev || !bias_dev || !out_dev) { set_error("%s: null pointer", who); return DIB_EINVAL; }
  if (h < 1 || w < 1) { set_error("%s: needs h, w >= 1 (got %d x %d)", who, h, w); return DIB_EINVAL; }
  if ((long long)h * w > DBL_MAX_PIXELS / 4) { set_error("%s: %lld source pixels, more than 2^28", who, (long long)h * w); return DIB_EINVAL; }
  if (!aligned16(in_dev) || !aligned16(out_dev) || ((uintptr_t)bias_dev & 3)) { set_error("%s: needs 16-byte aligned tensors", who); return DIB_EINVAL; }
  hipLaunchKernelGGL(deblur_shuffle_concat_kernel<T>, dim3(blocks_for((long long)h * w)), dim3(DBL_LANES), 0, (hipStream_t)stream, in_dev, bias_dev,
                     out_dev, h, w);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

// vectors of four elements: 16 bytes of fp32, 8 bytes of Half
template <typename T>
static int finish(const char *who, const T *in_dev, const float *bias_dev, T *out_dev, int H, int W, int Hp, int Wp, void *stream) {
  constexpr uintptr_t elem = sizeof(T), vector = DBL_PIX * sizeof(T);
  if (!in_dev || !bias_dev || !out_dev) { set_error("%s: null pointer", who); return DIB_EINVAL; }
  if (H < 1 || W < 1) { set_error("%s: needs H, W >= 1 (got %d x %d)", who, H, W); return DIB_EINVAL; }
  if (Hp < H || Wp < W) { set_error("%s: the padded size %d x %d is smaller than the image %d x %d", who, Hp, Wp, H, W); return DIB_EINVAL; }
  if ((long long)Hp * Wp > DBL_MAX_PIXELS) { set_error("%s: the padded image has %lld pixels, more than 2^30", who, (long long)Hp * Wp); return DIB_EINVAL; }
  if ((((uintptr_t)in_dev | (uintptr_t)out_dev) & (elem - 1)) || ((uintptr_t)bias_dev & 3)) {
    set_error("%s: needs %d-byte aligned tensors and a 4-byte aligned bias", who, (int)elem);
    return DIB_EINVAL;
  }
  const int vec = ((Wp % DBL_PIX) == 0 && (uintptr_t)in_dev % vector == 0 ? 1 : 0) | ((W % DBL_PIX) == 0 && (uintptr_t)out_dev % vector == 0 ? 2 : 0);
  hipLaunchKernelGGL(deblur_finish_kernel<T>, dim3(blocks_for((long long)H * ((W + DBL_PIX - 1) / DBL_PIX))), dim3(DBL_LANES), 0, (hipStream_t)stream,
                     in_dev, bias_dev, out_dev, H, W, Wp, vec);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

}  // namespace dib

using namespace dib;

extern "C" int dib_deblur_pyramid(const void *in_dev, int dtype, int H, int W, int n_scales, float *const *levels_dev, void *stream) {
  return pyramid<float>("dib_deblur_pyramid", in_dev, dtype, H, W, n_scales, levels_dev, nullptr, stream);
}

extern "C" int dib_deblur_shuffle_concat(const float *in_dev, const float *bias_dev, float *out_dev, int h, int w, void *stream) {
  return shuffle_concat<float>("dib_deblur_shuffle_concat", in_dev, bias_dev, out_dev, h, w, stream);
}

extern "C" int dib_deblur_finish(const float *in_dev, const float *bias_dev, float *out_dev, int H, int W, int Hp, int Wp, void *stream) {
  return finish<float>("dib_deblur_finish", in_dev, bias_dev, out_dev, H, W, Hp, Wp, stream);
}

// The Half forms (include/dib.h): levels, convolution outputs and the image as raw 16-bit words, biases fp32 vectors of Half values.
extern "C" int dib_deblur_pyramid_f16(const void *in_dev, int dtype, int H, int W, int n_scales, void *const *levels_dev, float *work_dev,
                                      void *stream) {
  return pyramid<__half>("dib_deblur_pyramid_f16", in_dev, dtype, H, W, n_scales, (__half *const *)levels_dev, work_dev, stream);
}

extern "C" int dib_deblur_shuffle_concat_f16(const void *in_dev, const float *bias_dev, void *out_dev, int h, int w, void *stream) {
  return shuffle_concat<__half>("dib_deblur_shuffle_concat_f16", (const __half *)in_dev, bias_dev, (__half *)out_dev, h, w, stream);
}

extern "C" int dib_deblur_finish_f16(const void *in_dev, const float *bias_dev, void *out_dev, int H, int W, int Hp, int Wp, void *stream) {
  return finish<__half>("dib_deblur_finish_f16", (const __half *)in_dev, bias_dev, (__half *)out_dev, H, W, Hp, Wp, stream);
}
