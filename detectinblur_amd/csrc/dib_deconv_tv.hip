// The total-variation factor of regularised Richardson-Lucy (Dey et al. 2006; include/dib.h: dib_tv_weight, dib_rl_deconvolve_tv;
// models/deconvolve.py; evaluate.py --deconvolve_tv).  Per plane x of H x W, out = x * g with
//   dx[i, j] = x[i, j + 1] - x[i, j] (0 in the last column)      dy[i, j] = x[i + 1, j] - x[i, j] (0 in the last row)
//   n = sqrt(dx^2 + dy^2 + beta^2)      p = dx / n      r = dy / n
//   div[i, j] = (p[i, j] - p[i, j - 1]) + (r[i, j] - r[i - 1, j])      p[i, -1] = r[-1, j] = 0
//   g = 1 / (1 - lambda * div)
// all in fp32, every sum, difference and product rounded on its own (-ffp-contract=off) in the order of models/deconvolve.py's
// tv_weight_torch.  1 / n and g are the hardware's reciprocal square root and reciprocal (v_rsq_f32, v_rcp_f32: 1 ulp each) instead of
// IEEE sqrt and three IEEE divisions, whose expansions (some 50 of 77 vector instructions per pixel) made the pass compute-bound
// (profiles/deconvolve_tv.txt has both forms' times); rcp(1) is 1, so a flat neighbourhood still gives g = 1 exactly.  The tests
// hold the result to the float64 definition.
//
// Shape.  No LDS, no barrier: a wave is on its own.  Lane l of a wave owns column x0 - 1 + l of a strip of 8 rows; lanes 1 .. 62 are
// the 62 output columns of the strip, lane 0 is the left halo (only its p is used) and lane 63 the right halo (only its x is used).
// The wave walks rows i0 - 1 .. i0 + 7 from top to bottom -- row i0 - 1 for its r alone -- with one load per lane and row, ten rows of
// 64 consecutive words, issued ahead of their use.  x[i, j + 1] and p[i, j - 1] come from the neighbouring lane
// (__shfl_down / __shfl_up), x[i + 1, j] is the next row's register, r[i - 1, j] the previous row's result: every p, r and n is
// computed once per pixel (plus the halo: 64 / 62 * 9 / 8 = 1.16 of the minimum) and the seven stencil points of a pixel are one
// load.  Coordinates outside the plane are clamped into it for the load and the differences there are set to 0 as the definition
// says, so nothing outside the plane is ever read and the rules at the plane's four edges need no branch.  A workgroup is four such
// waves on top of each other: a tile of 62 columns x 32 rows; the grid is one dimension of tiles_x * tiles_y * C workgroups.
// HBM traffic: every pixel is stored once (4 B) and loaded once from HBM (4 B, or 2 B of Half); the halo loads (0.29 of the loads)
// are the neighbouring waves' own lines and come from L2.
// Occupancy, chosen: 8 waves per SIMD (launch bounds: at most 64 vector registers; no LDS): the ten loads a wave has in flight are
// 2.5 KB, 80 KB per CU at full occupancy.  tests/test_deconvolve_tv_resources.py holds both instantiations to this budget.
// No scratch, no atomics, no allocation; an ordinary stream-ordered launch (capturable).
#include <hip/hip_fp16.h>

#include "dib_deconv_tv.h"

namespace dib {
namespace {

constexpr int TV_TW = 62, TV_WAVE_ROWS = 8, TV_TH = 4 * TV_WAVE_ROWS;

__device__ __forceinline__ float tv_load(const float *p, size_t i) { return p[i]; }
__device__ __forceinline__ float tv_load(const __half *p, size_t i) { return __half2float(p[i]); }

// grid = tiles_x * tiles_y * C workgroups of 256 lanes; tile (tx, ty) of plane z is workgroup (z * tiles_y + ty) * tiles_x + tx
template <typename T>
__global__ __launch_bounds__(256, 8) void tv_weight_kernel(const T *__restrict__ x, float *__restrict__ out, int H, int W, int tiles_x,
                                                           int tiles_y, float lambda, float beta) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  int b = blockIdx.x;
  const int tx = b % tiles_x;
  b /= tiles_x;
  const int ty = b % tiles_y, z = b / tiles_y;
  const int i0 = ty * TV_TH + wave * TV_WAVE_ROWS;
  if (i0 >= H) return;      // the whole wave: no barrier follows
  const int c = tx * TV_TW - 1 + lane;
  const size_t plane = (size_t)z * H * W;
  const size_t col = (size_t)min(max(c, 0), W - 1);
  const bool dx_live = c >= 0 && c < W - 1;
  const float b2 = beta * beta;

  float row[TV_WAVE_ROWS + 2];      // rows i0 - 1 .. i0 + 8 of this lane's column, clamped into the plane
#pragma unroll
  for (int k = 0; k < TV_WAVE_ROWS + 2; ++k) {
    const int i = min(max(i0 - 1 + k, 0), H - 1);
    row[k] = tv_load(x, plane + (size_t)i * W + col);
  }
  float r_up = 0.f;
#pragma unroll
  for (int k = 0; k < TV_WAVE_ROWS + 1; ++k) {
    const int i = i0 - 1 + k;      // wave-uniform
    const float v = row[k];
    const float right = __shfl_down(v, 1);
    const float dx = dx_live ? right - v : 0.f;
    const float dy = (i >= 0 && i < H - 1) ? row[k + 1] - v : 0.f;
    const float inv_n = __builtin_amdgcn_rsqf(dx * dx + dy * dy + b2);      // >= beta^2 > 0
    const float p = dx * inv_n, r = dy * inv_n;
    const float p_left = __shfl_up(p, 1);
    if (k > 0) {
      const float div = (p - p_left) + (r - r_up);
      const float g = __builtin_amdgcn_rcpf(1.f - lambda * div);      // the denominator lies in (0.6, 1.4)
      if (i < H && lane >= 1 && lane <= TV_TW && c < W) out[plane + (size_t)i * W + c] = v * g;
    }
    r_up = r;
  }
}

}  // namespace

int tv_weight_launch(const void *x, int dtype, float *out, int C, int H, int W, float lambda, float beta, hipStream_t s) {
  const int tiles_x = (W + TV_TW - 1) / TV_TW, tiles_y = (H + TV_TH - 1) / TV_TH;
  const long long blocks = (long long)tiles_x * tiles_y * C;      // <= C H W < 2^31 - 1
  if (blocks > 0x7fffffffll) { set_error("dib_tv_weight: image %d x %d x %d is too large", C, H, W); return DIB_ESHAPE; }
  if (dtype == DIB_F16)
    hipLaunchKernelGGL(tv_weight_kernel<__half>, dim3((unsigned)blocks), dim3(256), 0, s, (const __half *)x, out, H, W, tiles_x, tiles_y, lambda, beta);
  else
    hipLaunchKernelGGL(tv_weight_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, (const float *)x, out, H, W, tiles_x, tiles_y, lambda, beta);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

}  // namespace dib

using namespace dib;

extern "C" int dib_tv_weight(const void *x_dev, int dtype, float *out_dev, int C, int H, int W, float tv_lambda, float tv_beta, void *stream) {
  if (!x_dev || !out_dev) { set_error("dib_tv_weight: null pointer"); return DIB_EINVAL; }
  if (dtype != DIB_F16 && dtype != DIB_F32) { set_error("dib_tv_weight: unknown image dtype %d", dtype); return DIB_EINVAL; }
  if (C <= 0 || H <= 0 || W <= 0) { set_error("dib_tv_weight: empty shape %d x %d x %d", C, H, W); return DIB_EINVAL; }
  if (!tv_params_ok(tv_lambda, tv_beta)) {
    set_error("dib_tv_weight: tv_lambda must lie in (0, 0.1] and tv_beta be positive and finite, got %g and %g", (double)tv_lambda, (double)tv_beta);
    return DIB_EINVAL;
  }
  const long long n = (long long)C * H * W;
  if (n >= 0x7fffffffll) { set_error("dib_tv_weight: image %d x %d x %d is too large", C, H, W); return DIB_ESHAPE; }
  const uintptr_t xa = (uintptr_t)x_dev, oa = (uintptr_t)out_dev;
  const uintptr_t xb = (uintptr_t)n * (dtype == DIB_F16 ? 2 : 4), ob = (uintptr_t)n * 4;
  if (xa < oa + ob && oa < xa + xb) { set_error("dib_tv_weight: x_dev and out_dev must not overlap"); return DIB_EINVAL; }
  return tv_weight_launch(x_dev, dtype, out_dev, C, H, W, tv_lambda, tv_beta, (hipStream_t)stream);
}
