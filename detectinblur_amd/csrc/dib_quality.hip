// Restoration quality of one image against another (include/dib.h: dib_image_quality; quality.py):
// mean squared error, PSNR and the SSIM of Wang et al. 2004 with the 11 x 11 Gaussian window (sigma 1.5), valid windows only, population
// moments -- skimage.metrics.structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False, channel_axis=0).
//
// Shape.  A workgroup of 256 lanes owns a 32 x 32 tile of windows of one plane (a window is named by its top-left pixel), that is a
// 42 x 42 tile of pixels of each image:
//   1. stage: both pixel tiles go through registers into LDS as fp32 minus a PIVOT, each pixel loaded once per workgroup (coordinates
//      past the image are clamped into it: such pixels reach only windows that are masked below).  The pivot of a tile is the mean of
//      its 1,764 pixels as staged (fp32, fixed order), one per image: variances and covariance do not depend on a shift that all pixels
//      of a window share, and the pivot is added back to the means (which pivot is this file's choice, not part of the contract of
//      include/dib.h).  Against a fixed shift by L / 2 this takes the cancellation of E[x x] - mu^2 on a flat region from ~ulp(L^2 / 4)
//      down to ~ulp(var): the L / 2 form is off by up to 1e-4 in SSIM on near-flat bright pairs (tests/test_quality.py prints it as
//      d_half).  The lane that loads pixel p of a and of b also adds (a - b)^2, from the values as read, to its fp32 partial when this
//      workgroup OWNS p: the 32 x 32 pixels at the tile's origin, and for the last tile column / row everything right of / below them:
//      exactly one owner each.
//   2. rows: for each of the 42 rows and 32 window columns the 11-tap sums of a, b, a a, b b and a b (fused multiply-adds, taps left to
//      right), six items per lane kept in registers until every lane is done reading the pixel tiles; the five 42 x 32 planes then
//      overwrite them (the same LDS: 26,880 B instead of 40,992).
//   3. columns: a lane owns window column (lane & 31) of four consecutive window rows: per plane 14 LDS reads feed 4 x 11 fused
//      multiply-adds (taps top to bottom); then S in fp32, added to the lane's fp32 partial where the window exists.
//   4. the two partials of the 256 lanes are added in fp64 in a fixed order (butterfly inside a wave, waves 0..3 in turn) and written
//      as two doubles {sum of S, sum of (a - b)^2} to work_dev[workgroup].
// A second launch of one workgroup adds the workgroups' doubles in a fixed order (lane l takes l, l + 256, ...; then a fixed tree)
// and writes {mse, psnr_db, ssim}.  No atomics, no allocation: the same bits from run to run, capturable.
// LDS reads are conflict-free: a half-wave reads 32 consecutive words of one row in every phase.
// Occupancy, chosen: 4 workgroups per CU = 4 waves per SIMD (launch bounds: at most 128 vector registers -- the six row-sum items a lane
// holds across the barrier are 30 of them, and at 96 the compiler spills; 4 x 26,976 B = 105 KB of the CU's 160 KB of LDS): the five
// barriers of a workgroup are covered by the other three.  tests/test_quality_resources.py holds every instantiation to this budget.
// A 3 x 800 x 1333 pair is 3,150 workgroups on 1,024 slots.
// The window.  g_k = round(2^24 exp(-(k - 5)^2 / 4.5) / sum) / 2^24 with the centre tap taking the residual, so that the eleven sum
// to exactly 1 in fp32 IN ANY ORDER (every partial sum is a multiple of 2^-24 below 1): a constant image has exactly constant means
// (for a constant whose products with 2^-24 are exact) and exactly zero variance.  |g_k - exact| <= 2.2e-8, the
// order of the fp32 rounding of the weights themselves.
#include <hip/hip_fp16.h>

#include <math.h>

#include "dib_common.h"

namespace dib {
namespace {

constexpr int Q_TW = 32, Q_TH = 32, Q_TAPS = 11, Q_HALO = Q_TAPS - 1;
constexpr int Q_IW = Q_TW + Q_HALO, Q_IH = Q_TH + Q_HALO;                 // 42 x 42 pixels per image
constexpr int Q_PIX = Q_IW * Q_IH, Q_ROWSUMS = Q_IH * Q_TW;               // 1,764 pixels; 1,344 row sums per plane
constexpr int Q_THREADS = 256, Q_STAGE_TRIPS = (Q_PIX + Q_THREADS - 1) / Q_THREADS, Q_ROW_TRIPS = (Q_ROWSUMS + Q_THREADS - 1) / Q_THREADS;
constexpr int Q_LANE_ROWS = Q_TH * Q_TW / Q_THREADS;                      // 4 windows per lane
constexpr int Q_LDS_WORDS = 5 * Q_ROWSUMS;
static_assert(2 * Q_PIX <= Q_LDS_WORDS, "the five planes of row sums overwrite the two pixel tiles");
static_assert(Q_TW == 32 && Q_THREADS / Q_TW * Q_LANE_ROWS == Q_TH, "a half-wave is one tile row wide; eight of them, four rows each");

__device__ __forceinline__ float q_weight(int k) {
  constexpr float G[Q_TAPS] = {17253.f / 16777216.f,   127486.f / 16777216.f,  603993.f / 16777216.f, 1834768.f / 16777216.f,
                               3573640.f / 16777216.f, 4462936.f / 16777216.f, 3573640.f / 16777216.f, 1834768.f / 16777216.f,
                               603993.f / 16777216.f,  127486.f / 16777216.f,  17253.f / 16777216.f};
  return G[k];
}

__device__ __forceinline__ float q_load(const float *p, size_t i) { return p[i]; }
__device__ __forceinline__ float q_load(const __half *p, size_t i) { return __half2float(p[i]); }

// sum over the wave's 64 lanes, the same order on every lane (xor butterfly): all lanes end with the same value
template <typename T>
__device__ __forceinline__ T q_wave_sum(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// grid = tiles_x * tiles_y * C workgroups, flat (a plane's tiles row by row); work: two doubles per workgroup
template <typename TA, typename TB>
__global__ __launch_bounds__(Q_THREADS, 4) void quality_tile_kernel(const TA *__restrict__ a, const TB *__restrict__ b, int H, int W, int tiles_x,
                                                                    int tiles_y, float c1, float c2, double *__restrict__ work) {
  __shared__ float lds[Q_LDS_WORDS];
  __shared__ double red[2 * Q_THREADS / 64];
  __shared__ float piv[2 * Q_THREADS / 64];
  const int tid = threadIdx.x;
  const int per_plane = tiles_x * tiles_y;
  const int plane_id = blockIdx.x / per_plane, t = blockIdx.x - plane_id * per_plane;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int x0 = tx * Q_TW, y0 = ty * Q_TH;
  const bool last_col = tx == tiles_x - 1, last_row = ty == tiles_y - 1;
  const size_t plane = (size_t)plane_id * H * W;
  float *pa = lds, *pb = lds + Q_PIX;
  float sq = 0.f, ss = 0.f;

  // 1. the two pixel tiles; the squared differences of the pixels this workgroup owns; each tile's mean as its pivot
  float va[Q_STAGE_TRIPS], vb[Q_STAGE_TRIPS];
  float suma = 0.f, sumb = 0.f;
#pragma unroll
  for (int it = 0; it < Q_STAGE_TRIPS; ++it) {
    const int p = tid + it * Q_THREADS;
    va[it] = vb[it] = 0.f;
    if (p < Q_PIX) {
      const int r = p / Q_IW, c = p - r * Q_IW;
      const int gy = y0 + r, gx = x0 + c;
      const size_t e = plane + (size_t)min(gy, H - 1) * W + min(gx, W - 1);
      va[it] = q_load(a, e);
      vb[it] = q_load(b, e);
      const float d = va[it] - vb[it];
      const bool owned = gy < H && gx < W && (c < Q_TW || last_col) && (r < Q_TH || last_row);
      sq += owned ? d * d : 0.f;
      suma += va[it];
      sumb += vb[it];
    }
  }
  suma = q_wave_sum(suma);
  sumb = q_wave_sum(sumb);
  if ((tid & 63) == 0) {
    piv[2 * (tid >> 6)] = suma;
    piv[2 * (tid >> 6) + 1] = sumb;
  }
  __syncthreads();
  const float pivot_a = (((piv[0] + piv[2]) + piv[4]) + piv[6]) / (float)Q_PIX, pivot_b = (((piv[1] + piv[3]) + piv[5]) + piv[7]) / (float)Q_PIX;
#pragma unroll
  for (int it = 0; it < Q_STAGE_TRIPS; ++it) {
    const int p = tid + it * Q_THREADS;
    if (p < Q_PIX) {
      pa[p] = va[it] - pivot_a;
      pb[p] = vb[it] - pivot_b;
    }
  }
  __syncthreads();

  // 2. the row sums of the five quantities, in registers until the pixel tiles are no longer read
  float h[Q_ROW_TRIPS][5];
#pragma unroll
  for (int it = 0; it < Q_ROW_TRIPS; ++it) {
    const int item = min(tid + it * Q_THREADS, Q_ROWSUMS - 1);      // (the last trip's idle lanes redo the last item and drop it)
    const int r = item >> 5, x = item & 31;
    const float *ra = pa + r * Q_IW + x, *rb = pb + r * Q_IW + x;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
    for (int k = 0; k < Q_TAPS; ++k) {
      const float g = q_weight(k), xa = ra[k], xb = rb[k];
      s0 = __builtin_fmaf(g, xa, s0);
      s1 = __builtin_fmaf(g, xb, s1);
      s2 = __builtin_fmaf(g, xa * xa, s2);
      s3 = __builtin_fmaf(g, xb * xb, s3);
      s4 = __builtin_fmaf(g, xa * xb, s4);
    }
    h[it][0] = s0; h[it][1] = s1; h[it][2] = s2; h[it][3] = s3; h[it][4] = s4;
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < Q_ROW_TRIPS; ++it) {
    const int item = tid + it * Q_THREADS;
    if (item < Q_ROWSUMS) {
#pragma unroll
      for (int q = 0; q < 5; ++q) lds[q * Q_ROWSUMS + item] = h[it][q];
    }
  }
  __syncthreads();

  // 3. the column sums of this lane's four windows, and S
  const int x = tid & 31, yg = (tid >> 5) * Q_LANE_ROWS;
  float m[5][Q_LANE_ROWS];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    float col[Q_LANE_ROWS + Q_HALO];
#pragma unroll
    for (int r = 0; r < Q_LANE_ROWS + Q_HALO; ++r) col[r] = lds[q * Q_ROWSUMS + (yg + r) * Q_TW + x];
#pragma unroll
    for (int j = 0; j < Q_LANE_ROWS; ++j) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < Q_TAPS; ++k) s = __builtin_fmaf(q_weight(k), col[j + k], s);
      m[q][j] = s;
    }
  }
#pragma unroll
  for (int j = 0; j < Q_LANE_ROWS; ++j) {
    const float ma = m[0][j], mb = m[1][j];                       // the means of the shifted images
    const float var_a = m[2][j] - ma * ma, var_b = m[3][j] - mb * mb, cab = m[4][j] - ma * mb;
    const float mua = ma + pivot_a, mub = mb + pivot_b;
    const float num = (2.f * (mua * mub) + c1) * (2.f * cab + c2);
    const float den = (mua * mua + mub * mub + c1) * (var_a + var_b + c2);
    const float S = num / den;
    const bool exists = x0 + x < W - Q_HALO && y0 + yg + j < H - Q_HALO;
    ss += exists ? S : 0.f;
  }

  // 4. the workgroup's two sums, in fp64
  const double ws = q_wave_sum((double)ss), wq = q_wave_sum((double)sq);
  if ((tid & 63) == 0) {
    red[2 * (tid >> 6)] = ws;
    red[2 * (tid >> 6) + 1] = wq;
  }
  __syncthreads();
  if (tid == 0) {
    work[2 * (size_t)blockIdx.x] = ((red[0] + red[2]) + red[4]) + red[6];
    work[2 * (size_t)blockIdx.x + 1] = ((red[1] + red[3]) + red[5]) + red[7];
  }
}

// one workgroup: lane l adds workgroups l, l + 256, ... in that order, then a fixed tree over the 256 lanes
__global__ __launch_bounds__(Q_THREADS) void quality_finish_kernel(const double *__restrict__ work, int n_groups, double n_pixels, double n_windows,
                                                                   double range, float *__restrict__ out) {
  __shared__ double rs[Q_THREADS], rq[Q_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0, q = 0.0;
  for (int i = tid; i < n_groups; i += Q_THREADS) {
    s += work[2 * (size_t)i];
    q += work[2 * (size_t)i + 1];
  }
  rs[tid] = s;
  rq[tid] = q;
  __syncthreads();
  for (int w = Q_THREADS / 2; w >= 1; w >>= 1) {
    if (tid < w) {
      rs[tid] += rs[tid + w];
      rq[tid] += rq[tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double mse = rq[0] / n_pixels;
    out[0] = (float)mse;
    out[1] = mse == 0.0 ? INFINITY : (float)(10.0 * log10(range * range / mse));      // a NaN mse compares unequal: NaN
    out[2] = (float)(rs[0] / n_windows);
  }
}

template <typename TA, typename TB>
int quality_launch(const void *a, const void *b, int C, int H, int W, float range, float *out, double *work, hipStream_t s) {
  const int tiles_x = (W - Q_HALO + Q_TW - 1) / Q_TW, tiles_y = (H - Q_HALO + Q_TH - 1) / Q_TH;
  const int groups = tiles_x * tiles_y * C;
  const float c1 = (0.01f * range) * (0.01f * range), c2 = (0.03f * range) * (0.03f * range);
  hipLaunchKernelGGL((quality_tile_kernel<TA, TB>), dim3(groups), dim3(Q_THREADS), 0, s, (const TA *)a, (const TB *)b, H, W, tiles_x, tiles_y,
                     c1, c2, work);
  DIB_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(quality_finish_kernel, dim3(1), dim3(Q_THREADS), 0, s, (const double *)work, groups, (double)C * H * W,
                     (double)C * (H - Q_HALO) * (W - Q_HALO), (double)range, out);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

// workgroups of the tile kernel (0 where the entry point refuses the shape): C H W < 2^31 bounds it
long long quality_groups(int C, int H, int W) {
  if (C < 1 || H < Q_TAPS || W < Q_TAPS || (long long)C * H * W >= 0x7fffffffll) return 0;
  return (long long)C * ((H - Q_HALO + Q_TH - 1) / Q_TH) * ((W - Q_HALO + Q_TW - 1) / Q_TW);
}

}  // namespace
}  // namespace dib

using namespace dib;

extern "C" size_t dib_image_quality_workspace_bytes(int C, int H, int W) { return (size_t)quality_groups(C, H, W) * 2 * sizeof(double); }

extern "C" int dib_image_quality(const void *a_dev, int a_dtype, const void *b_dev, int b_dtype, int C, int H, int W, float data_range,
                                 float *out_dev, void *work_dev, void *stream) {
  if (!a_dev || !b_dev || !out_dev || !work_dev) { set_error("dib_image_quality: null pointer"); return DIB_EINVAL; }
  if ((a_dtype != DIB_F16 && a_dtype != DIB_F32) || (b_dtype != DIB_F16 && b_dtype != DIB_F32)) {
    set_error("dib_image_quality: unknown image dtype %d / %d", a_dtype, b_dtype);
    return DIB_EINVAL;
  }
  if (C < 1 || H < 1 || W < 1) { set_error("dib_image_quality: empty shape %d x %d x %d", C, H, W); return DIB_EINVAL; }
  if (!(data_range > 0.f) || !isfinite(data_range)) {
    set_error("dib_image_quality: data_range must be positive and finite, got %g", (double)data_range);
    return DIB_EINVAL;
  }
  const long long n = (long long)C * H * W;
  if (H < Q_TAPS || W < Q_TAPS) {
    set_error("dib_image_quality: image %d x %d is smaller than the 11 x 11 window", H, W);
    return DIB_ESHAPE;
  }
  if (n >= 0x7fffffffll) { set_error("dib_image_quality: image %d x %d x %d is too large", C, H, W); return DIB_ESHAPE; }
  const uintptr_t a = (uintptr_t)a_dev, b = (uintptr_t)b_dev, o = (uintptr_t)out_dev, w = (uintptr_t)work_dev;
  const uintptr_t ea = a_dtype == DIB_F16 ? 2 : 4, eb = b_dtype == DIB_F16 ? 2 : 4;
  if (a % ea || b % eb || o % sizeof(float) || w % sizeof(double)) {
    set_error("dib_image_quality: misaligned pointer (images: their element type, out_dev: 4 bytes, work_dev: 8)");
    return DIB_EINVAL;
  }
  {   // the inputs are only read (they may be one another); what is written may overlap neither them nor each other
    const uintptr_t ab = (uintptr_t)n * ea, bb = (uintptr_t)n * eb, ob = 3 * sizeof(float), wb = dib_image_quality_workspace_bytes(C, H, W);
    if ((o < a + ab && a < o + ob) || (o < b + bb && b < o + ob) || (w < a + ab && a < w + wb) || (w < b + bb && b < w + wb) ||
        (o < w + wb && w < o + ob)) {
      set_error("dib_image_quality: out_dev and work_dev must not overlap an input or each other");
      return DIB_EINVAL;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  double *work = (double *)work_dev;
  if (a_dtype == DIB_F16) {
    return b_dtype == DIB_F16 ? quality_launch<__half, __half>(a_dev, b_dev, C, H, W, data_range, out_dev, work, s)
                              : quality_launch<__half, float>(a_dev, b_dev, C, H, W, data_range, out_dev, work, s);
  }
  return b_dtype == DIB_F16 ? quality_launch<float, __half>(a_dev, b_dev, C, H, W, data_range, out_dev, work, s)
                            : quality_launch<float, float>(a_dev, b_dev, C, H, W, data_range, out_dev, work, s);
}
