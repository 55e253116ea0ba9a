// Device pieces of the image-quality kernels that dib_quality.hip (one pair) and dib_restoration.hip (one sharp image against one or
// two candidates) share: tile geometry, the window, staging with the per-tile pivot, the 11-tap row and column sums, S of a window,
// the workgroup's fp64 reduction and the final fixed-order sum.  dib_restoration.hip promises the bits of dib_image_quality for every
// candidate, so the arithmetic of a pair -- which lane takes which pixel, tap order, where a fused multiply-add stands, the order of
// every sum -- is stated here once and both files call it; dib_quality.hip's header comment describes the phases.
#pragma once
#include <hip/hip_fp16.h>

#include <math.h>

#include "dib_common.h"

namespace dib {
namespace {

constexpr int Q_TW = 32, Q_TH = 32, Q_TAPS = 11, Q_HALO = Q_TAPS - 1;
constexpr int Q_IW = Q_TW + Q_HALO, Q_IH = Q_TH + Q_HALO;                 // 42 x 42 pixels per image
constexpr int Q_PIX = Q_IW * Q_IH, Q_ROWSUMS = Q_IH * Q_TW;               // 1,764 pixels; 1,344 row sums per plane
constexpr int Q_THREADS = 256, Q_WAVES = Q_THREADS / 64;
constexpr int Q_STAGE_TRIPS = (Q_PIX + Q_THREADS - 1) / Q_THREADS, Q_ROW_TRIPS = (Q_ROWSUMS + Q_THREADS - 1) / Q_THREADS;
constexpr int Q_LANE_ROWS = Q_TH * Q_TW / Q_THREADS;                      // 4 windows per lane
static_assert(Q_TW == 32 && Q_THREADS / Q_TW * Q_LANE_ROWS == Q_TH, "a half-wave is one tile row wide; eight of them, four rows each");
static_assert(Q_WAVES == 4, "the workgroup's sums are written out for four waves");

// round(2^24 g_k) / 2^24 with the centre tap taking the residual (dib_quality.hip's header comment, "The window")
constexpr float Q_G[Q_TAPS] = {17253.f / 16777216.f,   127486.f / 16777216.f,  603993.f / 16777216.f, 1834768.f / 16777216.f,
                               3573640.f / 16777216.f, 4462936.f / 16777216.f, 3573640.f / 16777216.f, 1834768.f / 16777216.f,
                               603993.f / 16777216.f,  127486.f / 16777216.f,  17253.f / 16777216.f};

__device__ __forceinline__ float q_weight(int k) {
  constexpr float G[Q_TAPS] = {Q_G[0], Q_G[1], Q_G[2], Q_G[3], Q_G[4], Q_G[5], Q_G[6], Q_G[7], Q_G[8], Q_G[9], Q_G[10]};
  return G[k];
}

__device__ __forceinline__ float q_load(const float *p, size_t i) { return p[i]; }
__device__ __forceinline__ float q_load(const __half *p, size_t i) { return __half2float(p[i]); }

// the 8-bit grey level of a pixel of a [0, 1] image: rint(clamp(255 x, 0, 255)), ties to even; a NaN stays a NaN
__device__ __forceinline__ float q_grey8(float x) { return x != x ? x : rintf(fminf(fmaxf(255.f * x, 0.f), 255.f)); }

// sum over the wave's 64 lanes, the same order on every lane (xor butterfly): all lanes end with the same value
template <typename T>
__device__ __forceinline__ T q_wave_sum(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// the tile of windows a workgroup owns: grid = tiles_x * tiles_y * C workgroups, flat (a plane's tiles row by row)
struct QTile {
  int x0, y0, H, W;
  bool last_col, last_row;
  size_t plane;
};

__device__ __forceinline__ QTile q_tile(int H, int W, int tiles_x, int tiles_y) {
  const int per_plane = tiles_x * tiles_y;
  const int plane_id = blockIdx.x / per_plane, t = blockIdx.x - plane_id * per_plane;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  QTile q;
  q.x0 = tx * Q_TW;
  q.y0 = ty * Q_TH;
  q.H = H;
  q.W = W;
  q.last_col = tx == tiles_x - 1;
  q.last_row = ty == tiles_y - 1;
  q.plane = (size_t)plane_id * H * W;
  return q;
}

// what phase 1 leaves in a lane's registers: its pixels of candidate a, of the sharp image b and (WITH_C) of a second candidate c,
// their fp32 sums in trip order, and the lane's fp32 partials of (a - b)^2 and (c - b)^2 over the pixels this workgroup OWNS
struct QStaged {
  float va[Q_STAGE_TRIPS], vb[Q_STAGE_TRIPS], vc[Q_STAGE_TRIPS];
  float sum_a, sum_b, sum_c, sq_a, sq_c;
};

// phase 1, reading: this lane's pixels of the 42 x 42 tile (coordinates past the image clamped into it), as grey levels when `grey8`;
// one address per pixel for all images, the squared differences from the values as read
template <bool WITH_C, typename TA, typename TB, typename TC>
__device__ __forceinline__ void q_stage_read(const TA *__restrict__ a, const TB *__restrict__ b, const TC *__restrict__ c, const QTile &q, bool grey8,
                                             QStaged &s) {
  const int tid = threadIdx.x;
  s.sum_a = s.sum_b = s.sum_c = s.sq_a = s.sq_c = 0.f;
#pragma unroll
  for (int it = 0; it < Q_STAGE_TRIPS; ++it) {
    const int p = tid + it * Q_THREADS;
    s.va[it] = s.vb[it] = s.vc[it] = 0.f;
    if (p < Q_PIX) {
      const int r = p / Q_IW, col = p - r * Q_IW;
      const int gy = q.y0 + r, gx = q.x0 + col;
      const size_t e = q.plane + (size_t)min(gy, q.H - 1) * q.W + min(gx, q.W - 1);
      const bool owned = gy < q.H && gx < q.W && (col < Q_TW || q.last_col) && (r < Q_TH || q.last_row);
      const float xa = q_load(a, e), xb = q_load(b, e);
      s.va[it] = grey8 ? q_grey8(xa) : xa;
      s.vb[it] = grey8 ? q_grey8(xb) : xb;
      const float d = s.va[it] - s.vb[it];
      s.sq_a += owned ? d * d : 0.f;
      s.sum_a += s.va[it];
      s.sum_b += s.vb[it];
      if (WITH_C) {
        const float xc = q_load(c, e);
        s.vc[it] = grey8 ? q_grey8(xc) : xc;
        const float dc = s.vc[it] - s.vb[it];
        s.sq_c += owned ? dc * dc : 0.f;
        s.sum_c += s.vc[it];
      }
    }
  }
}

// the pivot of image `slot` of `n`: piv[wave * n + slot] holds the waves' sums of its staged pixels
__device__ __forceinline__ float q_pivot(const float *piv, int slot, int n) {
  return (((piv[slot] + piv[n + slot]) + piv[2 * n + slot]) + piv[3 * n + slot]) / (float)Q_PIX;
}

// phase 1, writing: the pixel tile as fp32 minus its pivot
__device__ __forceinline__ void q_stage_write(float *tile, const float (&v)[Q_STAGE_TRIPS], float pivot) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int it = 0; it < Q_STAGE_TRIPS; ++it) {
    const int p = tid + it * Q_THREADS;
    if (p < Q_PIX) tile[p] = v[it] - pivot;
  }
}

// phase 2: the 11-tap row sums of this lane's items, taps left to right: h[it] = {a, b, a a, b b, a b}; without WITH_B the sums of b
// alone (items 1 and 3) are left as they are
template <bool WITH_B>
__device__ __forceinline__ void q_row_sums(const float *pa, const float *pb, float (&h)[Q_ROW_TRIPS][5]) {
  const int tid = threadIdx.x;
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
      if (WITH_B) s1 = __builtin_fmaf(g, xb, s1);
      s2 = __builtin_fmaf(g, xa * xa, s2);
      if (WITH_B) s3 = __builtin_fmaf(g, xb * xb, s3);
      s4 = __builtin_fmaf(g, xa * xb, s4);
    }
    // an item's five sums are complete here, before the next item's LDS reads are issued: left to itself the scheduler interleaves
    // the six items and the kernels spill at their 128-register budget (no instruction, no change to the arithmetic)
    asm volatile("" : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3), "+v"(s4));
    h[it][0] = s0; h[it][2] = s2; h[it][4] = s4;
    if (WITH_B) { h[it][1] = s1; h[it][3] = s3; }
  }
}

// item q of this lane's row sums into the 42 x 32 plane `dst`
__device__ __forceinline__ void q_row_write(float *dst, const float (&h)[Q_ROW_TRIPS][5], int q) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int it = 0; it < Q_ROW_TRIPS; ++it) {
    const int item = tid + it * Q_THREADS;
    if (item < Q_ROWSUMS) dst[item] = h[it][q];
  }
}

// phase 3: a lane owns window column (lane & 31) of four consecutive window rows; the column sums of one plane, taps top to bottom
__device__ __forceinline__ void q_col_sums(const float *plane, float (&m)[Q_LANE_ROWS]) {
  const int x = threadIdx.x & 31, yg = (threadIdx.x >> 5) * Q_LANE_ROWS;
  float col[Q_LANE_ROWS + Q_HALO];
#pragma unroll
  for (int r = 0; r < Q_LANE_ROWS + Q_HALO; ++r) col[r] = plane[(yg + r) * Q_TW + x];
#pragma unroll
  for (int j = 0; j < Q_LANE_ROWS; ++j) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < Q_TAPS; ++k) s = __builtin_fmaf(q_weight(k), col[j + k], s);
    m[j] = s;
  }
}

// phase 3: S of this lane's four windows from the five planes of row sums, added in fp32 where the window exists
__device__ __forceinline__ float q_window_sum(const float *pl_a, const float *pl_b, const float *pl_aa, const float *pl_bb, const float *pl_ab,
                                              const QTile &q, float pivot_a, float pivot_b, float c1, float c2) {
  const int x = threadIdx.x & 31, yg = (threadIdx.x >> 5) * Q_LANE_ROWS;
  float m[5][Q_LANE_ROWS];
  q_col_sums(pl_a, m[0]);
  q_col_sums(pl_b, m[1]);
  q_col_sums(pl_aa, m[2]);
  q_col_sums(pl_bb, m[3]);
  q_col_sums(pl_ab, m[4]);
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < Q_LANE_ROWS; ++j) {
    const float ma = m[0][j], mb = m[1][j];                       // the means of the shifted images
    const float var_a = m[2][j] - ma * ma, var_b = m[3][j] - mb * mb, cab = m[4][j] - ma * mb;
    const float mua = ma + pivot_a, mub = mb + pivot_b;
    const float num = (2.f * (mua * mub) + c1) * (2.f * cab + c2);
    const float den = (mua * mua + mub * mub + c1) * (var_a + var_b + c2);
    const float S = num / den;
    const bool exists = q.x0 + x < q.W - Q_HALO && q.y0 + yg + j < q.H - Q_HALO;
    ss += exists ? S : 0.f;
  }
  return ss;
}

// phase 4: the workgroup's two sums in fp64 (butterfly inside a wave, waves 0..3 in turn) as pair[0] = sum of S, pair[1] = sum of
// (a - b)^2.  red: 2 * Q_WAVES doubles of LDS that nobody else touches before the next barrier
__device__ __forceinline__ void q_group_sums(float ss, float sq, double *red, double *pair) {
  const int tid = threadIdx.x;
  const double ws = q_wave_sum((double)ss), wq = q_wave_sum((double)sq);
  if ((tid & 63) == 0) {
    red[2 * (tid >> 6)] = ws;
    red[2 * (tid >> 6) + 1] = wq;
  }
  __syncthreads();
  if (tid == 0) {
    pair[0] = ((red[0] + red[2]) + red[4]) + red[6];
    pair[1] = ((red[1] + red[3]) + red[5]) + red[7];
  }
}

// the final sum, one workgroup: lane l adds the pairs of workgroups l, l + 256, ... in that order (pair i at work[stride * i]), then a
// fixed tree over the 256 lanes: rs[0] = sum of S, rq[0] = sum of (a - b)^2, valid on lane 0.  Ends behind a barrier.
__device__ __forceinline__ void q_final_sums(const double *__restrict__ work, int n_groups, int stride, double *rs, double *rq) {
  const int tid = threadIdx.x;
  double s = 0.0, q = 0.0;
  for (int i = tid; i < n_groups; i += Q_THREADS) {
    s += work[(size_t)stride * i];
    q += work[(size_t)stride * i + 1];
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
}

// {mse, psnr_db, ssim} from the two sums
__device__ __forceinline__ void q_figures(double sum_s, double sum_q, double n_pixels, double n_windows, double range, float *out) {
  const double mse = sum_q / n_pixels;
  out[0] = (float)mse;
  out[1] = mse == 0.0 ? INFINITY : (float)(10.0 * log10(range * range / mse));      // a NaN mse compares unequal: NaN
  out[2] = (float)(sum_s / n_windows);
}

// C1 and C2 of Wang et al. for a data range, as fp32 products
__host__ __device__ __forceinline__ float q_c1(float range) { return (0.01f * range) * (0.01f * range); }
__host__ __device__ __forceinline__ float q_c2(float range) { return (0.03f * range) * (0.03f * range); }

// workgroups of the tile kernel (0 where the entry points refuse the shape): C H W < 2^31 bounds it
inline int q_tiles(int extent) { return (extent - Q_HALO + Q_TW - 1) / Q_TW; }
inline long long q_groups(int C, int H, int W) {
  if (C < 1 || H < Q_TAPS || W < Q_TAPS || (long long)C * H * W >= 0x7fffffffll) return 0;
  return (long long)C * q_tiles(H) * q_tiles(W);
}

}  // namespace
}  // namespace dib
