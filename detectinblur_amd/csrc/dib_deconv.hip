// Non-blind Richardson-Lucy deconvolution with the blur's own forward model (include/dib.h: dib_rl_deconvolve;
// models/deconvolve.py; evaluate.py --deconvolve_first).  Two sweeps of the tap table per iteration over fp32 planes:
//   A  x : (A  x)[i, j] = sum_t w_t * x[m (i - (r_t - o)), m (j - (c_t - o))]      the blur (dib_blur.hip), epilogue q = y / max(A x, eps)
//   A* q : (A* q)[i, j] = sum_t w_t * q[m'(i + (r_t - o)), m'(j + (c_t - o))]      offsets negated, epilogue x' = clamp(x * A* q, 0, 1)
// o = K / 2 - 1; m = map_coord (dib_common.h: the padding rule of manual_blur WITH the wrap row / column of its torch.roll), m' = the
// same rule without the wrap.  One kernel serves both (template <ADJ>).
//
// Shape.  A workgroup of 256 lanes owns a 64 x 32 tile of one plane: lane l of wave w owns column l of rows 8 w .. 8 w + 7, eight fp32
// accumulators kept in registers across the whole table.  It walks the table's segments (runs of row-major consecutive taps with a
// bounding box of at most 13 PSF rows x 25 columns, the blur's own unit); per segment it stages the tile plus that segment's halo --
// at most 44 rows x 88 columns of fp32, 15,488 B -- into LDS through the boundary rule (all 22 loads of a lane in flight at once), then
// runs the segment's taps: every wave loads 64 taps at a time, one per lane, and broadcasts them lane by lane (v_readlane), so a tap
// is two broadcasts, eight LDS reads and eight fused multiply-adds per lane, conflict-free (a wave reads 64 consecutive words of one
// window row), with no memory access between two taps.  A table compacted for the large LDS window
// (DIB_COMPACT_LARGE_WINDOW: boxes of up to 21 x 64) is served as it is: a box larger than the window is cut into windows of 13 x 25
// and each window runs the taps of the segment that fall into it (the others with weight 0).
// Occupancy, chosen: 8 workgroups per CU = 8 waves per SIMD (launch bounds: at most 64 vector registers; 8 x 15,488 B = 121 KB of the
// CU's 160 KB of LDS, at most 80 scalar registers): while one workgroup waits at a window's fill and its two barriers, the others'
// tap loops have the CU.  tests/test_deconvolve_resources.py holds every instantiation to this budget.
// No scratch, no atomics, no allocation; every launch is an ordinary stream-ordered one (capturable).
// Contract: y is finite (in [0, 1]) and eps large enough that y / eps is.  A lane past a segment's end, or whose tap lies in another
// window of its segment, multiplies weight 0 by a live window word instead of skipping it: a NaN or Inf there would reach output
// pixels that the definition's taps do not connect it with.  Not tested, not guarded.
#include <hip/hip_fp16.h>

#include "dib_common.h"
#include "dib_deconv_tv.h"

namespace dib {
namespace {

constexpr int RL_TW = 64, RL_TH = 32, RL_LANE_ROWS = 8;
constexpr int RL_WIN_ROWS = RL_TH + SEG_ROWS, RL_WIN_COLS = RL_TW + SEG_COLS, RL_PITCH = RL_WIN_COLS;      // 44 x 88 words
static_assert(RL_TW == 64 && RL_TH == 4 * RL_LANE_ROWS, "a wave is one tile row wide; four waves of eight rows each");
constexpr int RL_FILL_ROWS = RL_WIN_ROWS / 4, RL_TAP_UNROLL = 4;
static_assert(64 % RL_TAP_UNROLL == 0, "a trip of the tap loop stays inside the chunk's 64 lanes");
static_assert(RL_WIN_COLS <= 128 && RL_WIN_ROWS % 4 == 0, "the fill writes columns lane and 64 + lane of rows wave, wave + 4, ...");

__device__ __forceinline__ float rl_load(const float *p, size_t i) { return p[i]; }
__device__ __forceinline__ float rl_load(const __half *p, size_t i) { return __half2float(p[i]); }

// m' of the adjoint sweep: map_coord's padding rule without the wrap (there is no torch.roll to imitate)
__device__ __forceinline__ int map_coord_nowrap(int s, int n, int mode, bool &zero) {
  zero = false;
  if (mode == PAD_REFLECT) {
    if (s < 0) s = -s;
    if (s > n - 1) s = 2 * (n - 1) - s;
  } else if (mode == PAD_ZERO) {
    zero = (s < 0) || (s > n - 1);
  }
  return min(max(s, 0), n - 1);
}

// ADJ = false: out = epi / max(A src, eps)        (src = x_k, epi = y, out = q)
// ADJ = true : out = clamp(epi * A* src, 0, 1)    (src = q,   epi = x_k, out = x_{k+1})
// S / E: element types of src / epi (__half only for y itself: x_0 = y, and the ratio's numerator); psf_f16: the table's weights
// are fp16 bits (low half of the word) instead of fp32 bits.  grid = (ceil(W / 64), ceil(H / 32), C).
template <bool ADJ, typename S, typename E>
__global__ __launch_bounds__(256, 8) void rl_sweep_kernel(const S *__restrict__ src, const E *__restrict__ epi, float *__restrict__ out, int H,
                                                          int W, const int *__restrict__ tab, int K, int psf_f16, float eps) {
  __shared__ float win[RL_WIN_ROWS * RL_PITCH];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int x0 = blockIdx.x * RL_TW, y0 = blockIdx.y * RL_TH;
  const size_t plane = (size_t)blockIdx.z * H * W;
  const int o = K / 2 - 1, pa = K / 2, pb = K / 2 - 1, mode = pad_mode_for(K, H, W);
  const int nsegs = tab[HDR_NSEGS];
  const uint4 *segs = reinterpret_cast<const uint4 *>(tab + table_segs_off(K));
  const uint2 *taps = reinterpret_cast<const uint2 *>(tab + table_taps_off(K));
  const float *mine = win + wave * RL_LANE_ROWS * RL_PITCH + lane;      // this lane's column of its wave's first row, at tap offset 0
  float acc[RL_LANE_ROWS];
#pragma unroll
  for (int k = 0; k < RL_LANE_ROWS; ++k) acc[k] = 0.f;

  for (int s = 0; s < nsegs; ++s) {
    const uint4 sg = segs[s];
    const int t0 = (int)sg.x, t1 = (int)sg.y, r_first = (int)(sg.z >> 8), r_last = (int)(sg.z & 255), cmin = (int)(sg.w >> 8), cmax = (int)(sg.w & 255);
    // one window per 13 x 25 part of the segment's box: exactly one for a table of the standard geometry
    for (int rlo = r_first; rlo <= r_last; rlo += SEG_ROWS + 1) {
      const int rhi = min(rlo + SEG_ROWS, r_last);
      for (int clo = cmin; clo <= cmax; clo += SEG_COLS + 1) {
        const int chi = min(clo + SEG_COLS, cmax);
        // the window's first row / column as a virtual (un-padded) coordinate, and where tap (r, c) of output row i sits in it:
        //   A : source row i + o - r -> window row (i - y0) + (rhi - r);   A*: source row i - o + r -> window row (i - y0) + (r - rlo)
        const int vr0 = ADJ ? y0 - o + rlo : y0 + o - rhi, vc0 = ADJ ? x0 - o + clo : x0 + o - chi;
        bool zc0, zc1;
        const int sx0 = ADJ ? map_coord_nowrap(vc0 + lane, W, mode, zc0) : map_coord(vc0 + lane, W, pa, pb, mode, zc0);
        const int sx1 = ADJ ? map_coord_nowrap(vc0 + 64 + lane, W, mode, zc1) : map_coord(vc0 + 64 + lane, W, pa, pb, mode, zc1);
        uint2 chunk = taps[min(t0 + lane, t1 - 1)];      // the segment's first 64 taps, one per lane (below): in flight during the fill
        // the fill: every lane's loads (11 window rows x 2 columns) are issued before the first is waited for.  Rows and columns past the
        // window's extent (wrows, wcols) are filled too, from clamped coordinates: inside the image, inside the 44 x 88 words, never read
        float v0[RL_FILL_ROWS], v1[RL_FILL_ROWS];
#pragma unroll
        for (int it = 0; it < RL_FILL_ROWS; ++it) {
          bool zr;
          const int wr = wave + 4 * it;
          const int sy = ADJ ? map_coord_nowrap(vr0 + wr, H, mode, zr) : map_coord(vr0 + wr, H, pa, pb, mode, zr);
          const size_t row = plane + (size_t)sy * W;
          v0[it] = rl_load(src, row + sx0);
          v1[it] = rl_load(src, row + sx1);
          if (zr || zc0) v0[it] = 0.f;
          if (zr || zc1) v1[it] = 0.f;
        }
        __syncthreads();      // every wave is done reading the previous window
#pragma unroll
        for (int it = 0; it < RL_FILL_ROWS; ++it) {
          const int wr = wave + 4 * it;
          win[wr * RL_PITCH + lane] = v0[it];
          if (lane < RL_WIN_COLS - 64) win[wr * RL_PITCH + 64 + lane] = v1[it];
        }
        __syncthreads();
        // The taps, 64 at a time: lane l of every wave holds tap t + l of the chunk, decoded into the word offset of its source inside the
        // window and its fp32 weight; the tap loop broadcasts one lane's pair per tap (v_readlane: no memory access between two taps) and
        // runs four taps per trip.  A lane past the segment's end, or whose tap lies in another window of this segment, holds weight 0 on
        // the window's first word: the trips need no tail and no branch.
        for (int t = t0; t < t1; t += 64) {
          const uint2 tap = chunk;
          chunk = taps[min(t + 64 + lane, t1 - 1)];      // the next chunk's words, in flight during this one's loop
          const int r = (int)(tap.x >> 8), c = (int)(tap.x & 255);
          const bool live = t + lane < t1 && r >= rlo && r <= rhi && c >= clo && c <= chi;
          const float wt = psf_f16 ? __half2float(__ushort_as_half((unsigned short)(tap.y & 0xffff))) : __uint_as_float(tap.y);
          const int w_lane = live ? (int)__float_as_uint(wt) : 0;
          const int off_lane = live ? (ADJ ? (r - rlo) * RL_PITCH + (c - clo) : (rhi - r) * RL_PITCH + (chi - c)) : 0;
          const int n = min(64, t1 - t);
          for (int u = 0; u < n; u += RL_TAP_UNROLL) {
#pragma unroll
            for (int v = 0; v < RL_TAP_UNROLL; ++v) {
              const float w = __uint_as_float((unsigned)__builtin_amdgcn_readlane(w_lane, u + v));
              const float *p = mine + __builtin_amdgcn_readlane(off_lane, u + v);
#pragma unroll
              for (int k = 0; k < RL_LANE_ROWS; ++k) acc[k] = __builtin_fmaf(w, p[k * RL_PITCH], acc[k]);
            }
          }
        }
      }
    }
  }

  const int j = x0 + lane;
#pragma unroll
  for (int k = 0; k < RL_LANE_ROWS; ++k) {
    const int i = y0 + wave * RL_LANE_ROWS + k;
    if (i < H && j < W) {
      const size_t e = plane + (size_t)i * W + j;
      const float v = rl_load(epi, e);
      out[e] = ADJ ? fminf(fmaxf(v * acc[k], 0.f), 1.f) : v / fmaxf(acc[k], eps);
    }
  }
}

template <bool ADJ, typename S, typename E>
int rl_launch(const S *src, const E *epi, float *out, int C, int H, int W, const int *tab, int K, int psf_f16, float eps, hipStream_t s) {
  const dim3 grid((W + RL_TW - 1) / RL_TW, (H + RL_TH - 1) / RL_TH, C);
  hipLaunchKernelGGL((rl_sweep_kernel<ADJ, S, E>), grid, dim3(256), 0, s, src, epi, out, H, W, tab, K, psf_f16, eps);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

}  // namespace
}  // namespace dib

using namespace dib;

namespace {

// The refusals of both entries (`who` names the caller in the message); work_planes: the planes of C H W floats in work_dev
int rl_check(const char *who, const void *y_dev, int dtype, const float *out_dev, const float *work_dev, int C, int H, int W, const void *table_dev,
             int psf_dtype, int K, int iterations, float eps, int work_planes) {
  if (!y_dev || !out_dev || !work_dev || !table_dev) { set_error("%s: null pointer", who); return DIB_EINVAL; }
  if (dtype != DIB_F16 && dtype != DIB_F32) { set_error("%s: unknown image dtype %d", who, dtype); return DIB_EINVAL; }
  if (psf_dtype != DIB_F16 && psf_dtype != DIB_F32) { set_error("%s: unknown PSF dtype %d", who, psf_dtype); return DIB_EINVAL; }
  if (K != 128 && K != 256) { set_error("%s: K must be 128 or 256, got %d", who, K); return DIB_EINVAL; }
  if (C <= 0 || H <= 0 || W <= 0) { set_error("%s: empty shape %d x %d x %d", who, C, H, W); return DIB_EINVAL; }
  if (iterations < 1 || iterations > 1000) { set_error("%s: iterations must lie in 1..1000, got %d", who, iterations); return DIB_EINVAL; }
  if (!(eps > 0.f)) { set_error("%s: eps must be positive, got %g", who, (double)eps); return DIB_EINVAL; }
  const long long n = (long long)C * H * W;
  if (n >= 0x7fffffffll || C > 65535 || (H + RL_TH - 1) / RL_TH > 65535) {
    set_error("%s: image %d x %d x %d is too large", who, C, H, W);
    return DIB_ESHAPE;
  }
  {   // the three buffers are read and written in turn: none may overlap another
    const uintptr_t y = (uintptr_t)y_dev, o = (uintptr_t)out_dev, w = (uintptr_t)work_dev;
    const uintptr_t yb = (uintptr_t)n * (dtype == DIB_F16 ? 2 : 4), ob = (uintptr_t)n * 4, wb = (uintptr_t)n * 4 * work_planes;
    if ((y < o + ob && o < y + yb) || (y < w + wb && w < y + yb) || (o < w + wb && w < o + ob)) {
      set_error("%s: y_dev, out_dev and work_dev must not overlap", who);
      return DIB_EINVAL;
    }
  }
  // F.pad(mode='reflect') raises unless pad < dim: where the blur refuses the image, A is not defined
  if (K == 128 && !(H < 64 || W < 64) && (H == 64 || W == 64)) {
    set_error("Padding size should be less than the corresponding input dimension (image is %dx%d)", H, W);
    return DIB_ESHAPE;
  }
  return DIB_OK;
}

// The iteration of both entries.  xg == nullptr: x_{k+1} = clamp(x_k * A* q, 0, 1), two launches per iteration.  Otherwise xg is a
// third plane and x_{k+1} = clamp((x_k * g_k) * A* q, 0, 1): csrc/dib_deconv_tv.hip writes x_k * g_k there and sweep A* takes it as
// its epi plane, three launches per iteration.
int rl_iterate(const void *y_dev, int dtype, float *out_dev, float *q, float *spare, float *xg, int C, int H, int W, const int *tab, int pf,
               int K, int iterations, float eps, float tv_lambda, float tv_beta, hipStream_t s) {
  const __half *y16 = (const __half *)y_dev;
  const float *y32 = (const float *)y_dev;
  const float *x = nullptr;      // x_k for k >= 1 (x_0 = y itself, in its own type)
  for (int k = 0; k < iterations; ++k) {
    float *next = ((iterations - 1 - k) & 1) ? spare : out_dev;      // x_N lands in out_dev, x_{N-1} in the spare plane, ...
    int rc;
    if (xg) {
      rc = x ? tv_weight_launch(x, DIB_F32, xg, C, H, W, tv_lambda, tv_beta, s) : tv_weight_launch(y_dev, dtype, xg, C, H, W, tv_lambda, tv_beta, s);
      if (rc) return rc;
    }
    if (dtype == DIB_F16) {
      rc = x ? rl_launch<false>(x, y16, q, C, H, W, tab, K, pf, eps, s) : rl_launch<false>(y16, y16, q, C, H, W, tab, K, pf, eps, s);
      if (rc) return rc;
      if (xg) rc = rl_launch<true>((const float *)q, (const float *)xg, next, C, H, W, tab, K, pf, eps, s);
      else rc = x ? rl_launch<true>((const float *)q, x, next, C, H, W, tab, K, pf, eps, s) : rl_launch<true>((const float *)q, y16, next, C, H, W, tab, K, pf, eps, s);
    } else {
      rc = rl_launch<false>(x ? x : y32, y32, q, C, H, W, tab, K, pf, eps, s);
      if (rc) return rc;
      rc = rl_launch<true>((const float *)q, xg ? (const float *)xg : (x ? x : y32), next, C, H, W, tab, K, pf, eps, s);
    }
    if (rc) return rc;
    x = next;
  }
  return DIB_OK;
}

}  // namespace

extern "C" int dib_rl_deconvolve(const void *y_dev, int dtype, float *out_dev, float *work_dev, int C, int H, int W, const void *table_dev,
                                 int psf_dtype, int K, int iterations, float eps, void *stream) {
  const int rc = rl_check("dib_rl_deconvolve", y_dev, dtype, out_dev, work_dev, C, H, W, table_dev, psf_dtype, K, iterations, eps, 2);
  if (rc) return rc;
  const size_t n = (size_t)C * H * W;
  return rl_iterate(y_dev, dtype, out_dev, work_dev, work_dev + n, nullptr, C, H, W, (const int *)table_dev, psf_dtype == DIB_F16 ? 1 : 0, K,
                    iterations, eps, 0.f, 0.f, (hipStream_t)stream);
}

extern "C" int dib_rl_deconvolve_tv(const void *y_dev, int dtype, float *out_dev, float *work_dev, int C, int H, int W, const void *table_dev,
                                    int psf_dtype, int K, int iterations, float eps, float tv_lambda, float tv_beta, void *stream) {
  const int rc = rl_check("dib_rl_deconvolve_tv", y_dev, dtype, out_dev, work_dev, C, H, W, table_dev, psf_dtype, K, iterations, eps, 3);
  if (rc) return rc;
  if (!tv_params_ok(tv_lambda, tv_beta)) {
    set_error("dib_rl_deconvolve_tv: tv_lambda must lie in (0, 0.1] and tv_beta be positive and finite, got %g and %g", (double)tv_lambda,
              (double)tv_beta);
    return DIB_EINVAL;
  }
  const size_t n = (size_t)C * H * W;
  return rl_iterate(y_dev, dtype, out_dev, work_dev, work_dev + n, work_dev + 2 * n, C, H, W, (const int *)table_dev, psf_dtype == DIB_F16 ? 1 : 0,
                    K, iterations, eps, tv_lambda, tv_beta, (hipStream_t)stream);
}
