// Restoration quality of one or two candidates against one sharp image in one launch, folded into a per-cell accumulator on the device
// (include/dib.h: dib_restoration_quality; quality.py: restoration_quality, RestorationMeter; `evaluate.py --restoration_metrics`).
// The definition and the arithmetic of a pair are dib_quality.hip's -- candidate k's three figures are dib_image_quality(cand_k, ref)
// bit for bit -- because every phase is the same function of dib_quality_dev.h, called with the candidate as `a` and the sharp image
// as `b`.  What this file adds is the order of the phases.
//
// Shape.  A workgroup owns the same 32 x 32 tile of windows (42 x 42 pixels) of one plane as there:
//   1. stage: the sharp tile and every candidate tile are read once, all loads in flight together (as 8-bit grey levels under quantize8);
//      their pivots and the candidates' owned squared differences are formed from the registers.  The sharp tile and candidate 0's go
//      to LDS; candidate 1's pixels stay in registers (7 per lane) until candidate 0 is done.
//   2. candidate 0: rows (all five sums; the sharp image's two planes, mean and E[r r], go to LDS of their own and are formed ONCE),
//      columns, S, the workgroup's pair of doubles -- as in dib_quality.hip.
//   3. candidate 1: its tile replaces candidate 0's planes; rows of the three sums that involve it (the sharp TILE is still there for
//      the cross term), columns over its three planes and the two kept ones, S, its pair of doubles.
// LDS: sharp tile 7,056 B + its two planes 10,752 B + one candidate's three planes 16,128 B (they overwrite its tile) = 33,936 B, and
// 112 B of sums.  Occupancy, chosen: 4 workgroups per CU = 4 waves per SIMD, as dib_quality.hip (launch bounds: at most 128 vector
// registers; 4 x 34,048 B = 133 KB of the CU's 160 KB): the candidates run one after the other over the kept sharp tile.  The
// alternative that keeps all 2 + 3 K = 8 planes resident needs 43 KB and 48 row-sum registers per lane, which is 3 workgroups per CU;
// it is below behind -DDIB_RQ_RESIDENT and measured slower (profiles/restoration_sweep.txt: 84.2 us against 77.4 us per call).  No scratch: tests/test_restoration_metrics_resources.py holds every
// instantiation to this budget.
// The finish kernel (one workgroup) adds each candidate's pairs in dib_quality.hip's order, writes 3 K floats and, when an accumulator
// is given, lane 0 folds the fp32-ROUNDED figures into it: what a host loop over the per-image results would add.  Calls on one stream
// are ordered, so the fold needs no atomics; nothing allocates; the call is capturable and gives the same bytes from run to run.
#include "dib_quality_dev.h"

namespace dib {
namespace {

constexpr int RQ_MAX_K = 2;
constexpr int RQ_REF_PLANES = Q_PIX, RQ_CAND = Q_PIX + 2 * Q_ROWSUMS;      // word offsets: sharp tile | its planes b, b b | candidate
constexpr int RQ_LDS_WORDS = RQ_CAND + 3 * Q_ROWSUMS;
static_assert(Q_PIX <= 3 * Q_ROWSUMS, "a candidate's three planes of row sums overwrite its pixel tile");
static_assert(DIB_RQ_ACC_DOUBLES == 6, "n, n_identical, n_nonfinite, sum_mse, sum_psnr_db, sum_ssim");

// one candidate over the staged sharp tile: dib_quality.hip's tile kernel from the second half of its phase 1 on.  FIRST also forms
// the sharp image's two planes.  Starts with the candidate area free, ends with lane 0 having written pair[0..1].
template <bool FIRST>
__device__ __forceinline__ void rq_candidate(float *lds, double *red, const QTile &q, const float (&va)[Q_STAGE_TRIPS], float pivot_a, float pivot_b,
                                             float sq, float c1, float c2, double *pair) {
  float *tile_b = lds, *pl_b = lds + RQ_REF_PLANES, *pl_bb = pl_b + Q_ROWSUMS;
  float *tile_a = lds + RQ_CAND, *pl_a = tile_a, *pl_aa = pl_a + Q_ROWSUMS, *pl_ab = pl_aa + Q_ROWSUMS;
  q_stage_write(tile_a, va, pivot_a);
  __syncthreads();
  float h[Q_ROW_TRIPS][5];
  q_row_sums<FIRST>(tile_a, tile_b, h);
  __syncthreads();
  q_row_write(pl_a, h, 0);
  q_row_write(pl_aa, h, 2);
  q_row_write(pl_ab, h, 4);
  if (FIRST) {
    q_row_write(pl_b, h, 1);
    q_row_write(pl_bb, h, 3);
  }
  __syncthreads();
  const float ss = q_window_sum(pl_a, pl_b, pl_aa, pl_bb, pl_ab, q, pivot_a, pivot_b, c1, c2);
  q_group_sums(ss, sq, red, pair);
}

// grid as quality_tile_kernel's; work: 2 K doubles per workgroup, candidate k's pair at [2 K g + 2 k]
template <int K, typename TR, typename TC0, typename TC1>
__global__ __launch_bounds__(Q_THREADS, 4) void restoration_tile_kernel(const TR *__restrict__ ref, const TC0 *__restrict__ cand0,
                                                                        const TC1 *__restrict__ cand1, int H, int W, int tiles_x, int tiles_y,
                                                                        int grey8, float c1, float c2, double *__restrict__ work) {
  __shared__ float lds[RQ_LDS_WORDS];
  __shared__ double red[2 * Q_WAVES];
  __shared__ float piv[3 * Q_WAVES];
  const int tid = threadIdx.x;
  const QTile q = q_tile(H, W, tiles_x, tiles_y);

  QStaged s;
  q_stage_read<K == 2>(cand0, ref, cand1, q, grey8 != 0, s);
  const float sum0 = q_wave_sum(s.sum_a), sumr = q_wave_sum(s.sum_b), sum1 = K == 2 ? q_wave_sum(s.sum_c) : 0.f;
  if ((tid & 63) == 0) {
    piv[3 * (tid >> 6)] = sum0;
    piv[3 * (tid >> 6) + 1] = sumr;
    piv[3 * (tid >> 6) + 2] = sum1;
  }
  __syncthreads();
  const float pivot_0 = q_pivot(piv, 0, 3), pivot_r = q_pivot(piv, 1, 3), pivot_1 = q_pivot(piv, 2, 3);
  q_stage_write(lds, s.vb, pivot_r);

  double *pair = work + 2 * (size_t)K * blockIdx.x;
  rq_candidate<true>(lds, red, q, s.va, pivot_0, pivot_r, s.sq_a, c1, c2, pair);
  if (K == 2) {
    __syncthreads();      // candidate 0's planes and `red` have been read
    rq_candidate<false>(lds, red, q, s.vc, pivot_1, pivot_r, s.sq_c, c1, c2, pair + 2);
  }
}

#ifdef DIB_RQ_RESIDENT
// The alternative profiles/restoration_sweep.txt measures against the kernel above (built only with -DDIB_RQ_RESIDENT, K = 2): all
// 2 + 3 K = 8 row-sum planes resident (43,008 B; they overwrite the three pixel tiles), both candidates' rows in one phase (48 live
// row-sum registers per lane), one set of barriers instead of two -- and 3 workgroups per CU instead of 4.  The same functions, the same bits.
template <typename TR, typename TC0, typename TC1>
__global__ __launch_bounds__(Q_THREADS, 3) void restoration_tile_resident_kernel(const TR *__restrict__ ref, const TC0 *__restrict__ cand0,
                                                                                 const TC1 *__restrict__ cand1, int H, int W, int tiles_x,
                                                                                 int tiles_y, int grey8, float c1, float c2,
                                                                                 double *__restrict__ work) {
  __shared__ float lds[8 * Q_ROWSUMS];
  __shared__ double red[2 * Q_WAVES];
  __shared__ float piv[3 * Q_WAVES];
  static_assert(3 * Q_PIX <= 8 * Q_ROWSUMS, "the eight planes overwrite the three pixel tiles");
  const int tid = threadIdx.x;
  const QTile q = q_tile(H, W, tiles_x, tiles_y);
  QStaged s;
  q_stage_read<true>(cand0, ref, cand1, q, grey8 != 0, s);
  const float sum0 = q_wave_sum(s.sum_a), sumr = q_wave_sum(s.sum_b), sum1 = q_wave_sum(s.sum_c);
  if ((tid & 63) == 0) {
    piv[3 * (tid >> 6)] = sum0;
    piv[3 * (tid >> 6) + 1] = sumr;
    piv[3 * (tid >> 6) + 2] = sum1;
  }
  __syncthreads();
  const float pivot_0 = q_pivot(piv, 0, 3), pivot_r = q_pivot(piv, 1, 3), pivot_1 = q_pivot(piv, 2, 3);
  float *tile_b = lds, *tile_0 = lds + Q_PIX, *tile_1 = lds + 2 * Q_PIX;
  q_stage_write(tile_b, s.vb, pivot_r);
  q_stage_write(tile_0, s.va, pivot_0);
  q_stage_write(tile_1, s.vc, pivot_1);
  __syncthreads();
  float h0[Q_ROW_TRIPS][5], h1[Q_ROW_TRIPS][5];
  q_row_sums<true>(tile_0, tile_b, h0);
  q_row_sums<false>(tile_1, tile_b, h1);
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 5; ++p) q_row_write(lds + p * Q_ROWSUMS, h0, p);
  q_row_write(lds + 5 * Q_ROWSUMS, h1, 0);
  q_row_write(lds + 6 * Q_ROWSUMS, h1, 2);
  q_row_write(lds + 7 * Q_ROWSUMS, h1, 4);
  __syncthreads();
  const float *pl = lds;
  const float ss0 = q_window_sum(pl, pl + Q_ROWSUMS, pl + 2 * Q_ROWSUMS, pl + 3 * Q_ROWSUMS, pl + 4 * Q_ROWSUMS, q, pivot_0, pivot_r, c1, c2);
  const float ss1 = q_window_sum(pl + 5 * Q_ROWSUMS, pl + Q_ROWSUMS, pl + 6 * Q_ROWSUMS, pl + 3 * Q_ROWSUMS, pl + 7 * Q_ROWSUMS, q, pivot_1,
                                 pivot_r, c1, c2);
  double *pair = work + 4 * (size_t)blockIdx.x;
  q_group_sums(ss0, s.sq_a, red, pair);
  __syncthreads();
  q_group_sums(ss1, s.sq_c, red, pair + 2);
}
#endif

// one workgroup: per candidate dib_quality.hip's final sum; lane 0 writes the three figures and folds them into the accumulator
__global__ __launch_bounds__(Q_THREADS) void restoration_finish_kernel(const double *__restrict__ work, int n_groups, int K, double n_pixels,
                                                                       double n_windows, double range, float *__restrict__ out,
                                                                       double *__restrict__ acc) {
  __shared__ double rs[Q_THREADS], rq[Q_THREADS];
  for (int k = 0; k < K; ++k) {
    q_final_sums(work + 2 * k, n_groups, 2 * K, rs, rq);
    if (threadIdx.x == 0) {
      float f[3];
      q_figures(rs[0], rq[0], n_pixels, n_windows, range, f);
      out[3 * k] = f[0];
      out[3 * k + 1] = f[1];
      out[3 * k + 2] = f[2];
      if (acc) {      // {n, n_identical, n_nonfinite, sum_mse, sum_psnr_db, sum_ssim}: the figures as a reader of `out` sees them
        double *a = acc + DIB_RQ_ACC_DOUBLES * k;
        if (!isfinite(f[0]) || !isfinite(f[2])) {
          a[2] += 1.0;
        } else {
          a[0] += 1.0;
          a[3] += (double)f[0];
          a[5] += (double)f[2];
          if (f[0] == 0.f) a[1] += 1.0;      // +inf dB: counted, left out of the PSNR sum
          else a[4] += (double)f[1];
        }
      }
    }
    __syncthreads();
  }
}

template <int K, typename TR, typename TC0, typename TC1>
int restoration_launch(const void *ref, const void *const *cand, int C, int H, int W, int grey8, float range, float *out, double *acc,
                       double *work, hipStream_t s) {
  const int tiles_x = q_tiles(W), tiles_y = q_tiles(H);
  const int groups = tiles_x * tiles_y * C;
#ifdef DIB_RQ_RESIDENT
  if (K == 2)
    hipLaunchKernelGGL((restoration_tile_resident_kernel<TR, TC0, TC1>), dim3(groups), dim3(Q_THREADS), 0, s, (const TR *)ref,
                       (const TC0 *)cand[0], (const TC1 *)cand[1], H, W, tiles_x, tiles_y, grey8, q_c1(range), q_c2(range), work);
  else
#endif
  hipLaunchKernelGGL((restoration_tile_kernel<K, TR, TC0, TC1>), dim3(groups), dim3(Q_THREADS), 0, s, (const TR *)ref, (const TC0 *)cand[0],
                     (const TC1 *)cand[K - 1], H, W, tiles_x, tiles_y, grey8, q_c1(range), q_c2(range), work);
  DIB_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(restoration_finish_kernel, dim3(1), dim3(Q_THREADS), 0, s, (const double *)work, groups, K, (double)C * H * W,
                     (double)C * (H - Q_HALO) * (W - Q_HALO), (double)range, out, acc);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

// K = 1: the second candidate's slot repeats the first one's type and is never read (four instantiations; K = 2: eight)
template <typename TR, typename TC0>
int restoration_launch_c1(int dt1, const void *ref, const void *const *cand, int K, int C, int H, int W, int grey8, float range, float *out,
                          double *acc, double *work, hipStream_t s) {
  if (K == 1) return restoration_launch<1, TR, TC0, TC0>(ref, cand, C, H, W, grey8, range, out, acc, work, s);
  return dt1 == DIB_F16 ? restoration_launch<2, TR, TC0, __half>(ref, cand, C, H, W, grey8, range, out, acc, work, s)
                        : restoration_launch<2, TR, TC0, float>(ref, cand, C, H, W, grey8, range, out, acc, work, s);
}

template <typename TR>
int restoration_launch_c0(int dt0, int dt1, const void *ref, const void *const *cand, int K, int C, int H, int W, int grey8, float range, float *out,
                          double *acc, double *work, hipStream_t s) {
  return dt0 == DIB_F16 ? restoration_launch_c1<TR, __half>(dt1, ref, cand, K, C, H, W, grey8, range, out, acc, work, s)
                        : restoration_launch_c1<TR, float>(dt1, ref, cand, K, C, H, W, grey8, range, out, acc, work, s);
}

bool overlap(uintptr_t a, uintptr_t an, uintptr_t b, uintptr_t bn) { return a < b + bn && b < a + an; }

}  // namespace
}  // namespace dib

using namespace dib;

extern "C" size_t dib_restoration_quality_workspace_bytes(int K, int C, int H, int W) {
  if (K < 1 || K > RQ_MAX_K) return 0;
  return (size_t)q_groups(C, H, W) * 2 * K * sizeof(double);
}

extern "C" int dib_restoration_quality(const void *ref_dev, int ref_dtype, const void *const *cand_dev, const int *cand_dtype, int K, int C, int H,
                                       int W, int quantize8, float data_range, float *out_dev, double *acc_dev, void *work_dev, void *stream) {
  if (K < 1 || K > RQ_MAX_K) { set_error("dib_restoration_quality: K = %d candidates, 1 or 2 are supported", K); return DIB_EINVAL; }
  if (!ref_dev || !cand_dev || !cand_dtype || !out_dev || !work_dev) { set_error("dib_restoration_quality: null pointer"); return DIB_EINVAL; }
  for (int k = 0; k < K; ++k) {
    if (!cand_dev[k]) { set_error("dib_restoration_quality: null pointer (candidate %d)", k); return DIB_EINVAL; }
  }
  if (ref_dtype != DIB_F16 && ref_dtype != DIB_F32) { set_error("dib_restoration_quality: unknown image dtype %d", ref_dtype); return DIB_EINVAL; }
  for (int k = 0; k < K; ++k) {
    if (cand_dtype[k] != DIB_F16 && cand_dtype[k] != DIB_F32) {
      set_error("dib_restoration_quality: unknown image dtype %d (candidate %d)", cand_dtype[k], k);
      return DIB_EINVAL;
    }
  }
  if (C < 1 || H < 1 || W < 1) { set_error("dib_restoration_quality: empty shape %d x %d x %d", C, H, W); return DIB_EINVAL; }
  if (!(data_range > 0.f) || !isfinite(data_range)) {
    set_error("dib_restoration_quality: data_range must be positive and finite, got %g", (double)data_range);
    return DIB_EINVAL;
  }
  if (quantize8 && data_range != 1.f) {
    set_error("dib_restoration_quality: quantize8 takes images in [0, 1]: data_range must be 1, got %g", (double)data_range);
    return DIB_EINVAL;
  }
  const long long n = (long long)C * H * W;
  if (H < Q_TAPS || W < Q_TAPS) {
    set_error("dib_restoration_quality: image %d x %d is smaller than the 11 x 11 window", H, W);
    return DIB_ESHAPE;
  }
  if (n >= 0x7fffffffll) { set_error("dib_restoration_quality: image %d x %d x %d is too large", C, H, W); return DIB_ESHAPE; }
  // what is read: the sharp image and the candidates (they may be one another); what is written: out, acc, work
  uintptr_t in[1 + RQ_MAX_K], in_bytes[1 + RQ_MAX_K];
  in[0] = (uintptr_t)ref_dev;
  in_bytes[0] = (uintptr_t)n * (ref_dtype == DIB_F16 ? 2 : 4);
  bool misaligned = in[0] % (ref_dtype == DIB_F16 ? 2 : 4) != 0;
  for (int k = 0; k < K; ++k) {
    const uintptr_t e = cand_dtype[k] == DIB_F16 ? 2 : 4;
    in[1 + k] = (uintptr_t)cand_dev[k];
    in_bytes[1 + k] = (uintptr_t)n * e;
    misaligned = misaligned || in[1 + k] % e != 0;
  }
  const uintptr_t wr[3] = {(uintptr_t)out_dev, (uintptr_t)acc_dev, (uintptr_t)work_dev};
  const uintptr_t wr_bytes[3] = {3 * K * sizeof(float), acc_dev ? DIB_RQ_ACC_DOUBLES * K * sizeof(double) : 0,
                                 dib_restoration_quality_workspace_bytes(K, C, H, W)};
  if (misaligned || wr[0] % sizeof(float) || wr[1] % sizeof(double) || wr[2] % sizeof(double)) {
    set_error("dib_restoration_quality: misaligned pointer (images: their element type, out_dev: 4 bytes, acc_dev and work_dev: 8)");
    return DIB_EINVAL;
  }
  for (int i = 0; i < 3; ++i) {
    if (!wr_bytes[i]) continue;
    bool bad = false;
    for (int j = 0; j <= K; ++j) bad = bad || overlap(wr[i], wr_bytes[i], in[j], in_bytes[j]);
    for (int j = i + 1; j < 3; ++j) bad = bad || (wr_bytes[j] && overlap(wr[i], wr_bytes[i], wr[j], wr_bytes[j]));
    if (bad) {
      set_error("dib_restoration_quality: out_dev, acc_dev and work_dev must not overlap an input or each other");
      return DIB_EINVAL;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  const float range = quantize8 ? 255.f : data_range;
  const int dt0 = cand_dtype[0], dt1 = cand_dtype[K - 1];      // K = 1: the second slot repeats the first and is never read
  return ref_dtype == DIB_F16
             ? restoration_launch_c0<__half>(dt0, dt1, ref_dev, cand_dev, K, C, H, W, quantize8 != 0, range, out_dev, acc_dev, (double *)work_dev, s)
             : restoration_launch_c0<float>(dt0, dt1, ref_dev, cand_dev, K, C, H, W, quantize8 != 0, range, out_dev, acc_dev, (double *)work_dev, s);
}
