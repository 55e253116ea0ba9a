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
// The phases themselves are in dib_quality_dev.h: dib_restoration.hip (one sharp image against one or two candidates in one launch)
// promises this file's bits for every candidate and calls the same functions.
#include "dib_quality_dev.h"

namespace dib {
namespace {

constexpr int Q_LDS_WORDS = 5 * Q_ROWSUMS;
static_assert(2 * Q_PIX <= Q_LDS_WORDS, "the five planes of row sums overwrite the two pixel tiles");
// the window as stated above, against the shared table
static_assert(Q_G[0] == 17253.f / 16777216.f && Q_G[1] == 127486.f / 16777216.f && Q_G[2] == 603993.f / 16777216.f &&
                  Q_G[3] == 1834768.f / 16777216.f && Q_G[4] == 3573640.f / 16777216.f && Q_G[5] == 4462936.f / 16777216.f &&
                  Q_G[6] == Q_G[4] && Q_G[7] == Q_G[3] && Q_G[8] == Q_G[2] && Q_G[9] == Q_G[1] && Q_G[10] == Q_G[0],
              "round(2^24 g_k) / 2^24, symmetric");

// grid = tiles_x * tiles_y * C workgroups, flat (a plane's tiles row by row); work: two doubles per workgroup
template <typename TA, typename TB>
__global__ __launch_bounds__(Q_THREADS, 4) void quality_tile_kernel(const TA *__restrict__ a, const TB *__restrict__ b, int H, int W, int tiles_x,
                                                                    int tiles_y, float c1, float c2, double *__restrict__ work) {
  __shared__ float lds[Q_LDS_WORDS];
  __shared__ double red[2 * Q_WAVES];
  __shared__ float piv[2 * Q_WAVES];
  const int tid = threadIdx.x;
  const QTile q = q_tile(H, W, tiles_x, tiles_y);
  float *pa = lds, *pb = lds + Q_PIX;

  // 1. the two pixel tiles; the squared differences of the pixels this workgroup owns; each tile's mean as its pivot
  QStaged s;
  q_stage_read<false>(a, b, b, q, false, s);
  const float sq = s.sq_a;
  const float suma = q_wave_sum(s.sum_a), sumb = q_wave_sum(s.sum_b);
  if ((tid & 63) == 0) {
    piv[2 * (tid >> 6)] = suma;
    piv[2 * (tid >> 6) + 1] = sumb;
  }
  __syncthreads();
  const float pivot_a = q_pivot(piv, 0, 2), pivot_b = q_pivot(piv, 1, 2);
  q_stage_write(pa, s.va, pivot_a);
  q_stage_write(pb, s.vb, pivot_b);
  __syncthreads();

  // 2. the row sums of the five quantities, in registers until the pixel tiles are no longer read
  float h[Q_ROW_TRIPS][5];
  q_row_sums<true>(pa, pb, h);
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 5; ++p) q_row_write(lds + p * Q_ROWSUMS, h, p);
  __syncthreads();

  // 3. the column sums of this lane's four windows, and S
  const float ss = q_window_sum(lds, lds + Q_ROWSUMS, lds + 2 * Q_ROWSUMS, lds + 3 * Q_ROWSUMS, lds + 4 * Q_ROWSUMS, q, pivot_a, pivot_b, c1, c2);

  // 4. the workgroup's two sums, in fp64
  q_group_sums(ss, sq, red, work + 2 * (size_t)blockIdx.x);
}

// one workgroup: lane l adds workgroups l, l + 256, ... in that order, then a fixed tree over the 256 lanes
__global__ __launch_bounds__(Q_THREADS) void quality_finish_kernel(const double *__restrict__ work, int n_groups, double n_pixels, double n_windows,
                                                                   double range, float *__restrict__ out) {
  __shared__ double rs[Q_THREADS], rq[Q_THREADS];
  q_final_sums(work, n_groups, 2, rs, rq);
  if (threadIdx.x == 0) q_figures(rs[0], rq[0], n_pixels, n_windows, range, out);
}

template <typename TA, typename TB>
int quality_launch(const void *a, const void *b, int C, int H, int W, float range, float *out, double *work, hipStream_t s) {
  const int tiles_x = q_tiles(W), tiles_y = q_tiles(H);
  const int groups = tiles_x * tiles_y * C;
  hipLaunchKernelGGL((quality_tile_kernel<TA, TB>), dim3(groups), dim3(Q_THREADS), 0, s, (const TA *)a, (const TB *)b, H, W, tiles_x, tiles_y,
                     q_c1(range), q_c2(range), work);
  DIB_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(quality_finish_kernel, dim3(1), dim3(Q_THREADS), 0, s, (const double *)work, groups, (double)C * H * W,
                     (double)C * (H - Q_HALO) * (W - Q_HALO), (double)range, out);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

}  // namespace
}  // namespace dib

using namespace dib;

extern "C" size_t dib_image_quality_workspace_bytes(int C, int H, int W) { return (size_t)q_groups(C, H, W) * 2 * sizeof(double); }

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
