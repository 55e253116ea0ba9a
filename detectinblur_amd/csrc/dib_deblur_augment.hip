// The value half of DeepDeblur's patch augmentation (reference models/deblur/dataCommon.py: augment :72-87 with change_saturation,
// add_noise :43-54), fused with the data movement of dib_deblur_patches (the patch map of dib_deblur_patch.h: crop, flips, transpose,
// channel order).  Both steps are pointwise per pixel, so they commute with that movement and ride in its launch: one lane per output
// pixel loads its three channels through the composed index map, and stores three fp32 values.  As torch ops the same chain is about
// twenty small kernels per list.  HBM-bound; no LDS, no scratch, no atomics, caller's stream (capturable).
//
// Per pixel, on the 0..255 scale in fp32, every multiply, subtract and add rounded on its own (-ffp-contract=off):
//   1. q_c = quantise(v_c)                              dib_deblur.hip's step 1 (models/deblur.quantise): the 8-bit file the reference reads
//   2. m = max(q_0, q_1, q_2);  x_c = min(max(m - a * (m - q_c), 0), 255)
//                                                       = hsv2rgb(rgb2hsv(img) with S *= a).clip(0, 1) * 255 (:83-87) WITHOUT the hue:
//                                                       scaling S moves every channel along the line to the pixel's maximum, which V
//                                                       keeps.  m - q_c is an exact integer, so a == 1 returns q_c exactly.
//   3. sigma != 0:  x_c = min(max(x_c + sigma * n_i, 0), 255)      (:50-52)
//                                                       n_i = normal_at(i, key0, key1), i = (c * ps + y) * ps + x the element's index
//                                                       in the image's OUTPUT patch: the field does not depend on the flips
//   4. g_c = rintf(x_c);  out = g_c / 255.0f            quantise(g / 255.0f) == g for all 256 levels, so the pyramid kernels that
//                                                       follow see exactly g
// models/deblur_train.py (augment_patches_torch) restates this op for op; tests/test_deblur_augment*.py hold both to a float64 HSV
// round trip.
#include "dib_deblur_patch.h"
#include "dib_philox_dev.h"
#include <hip/hip_fp16.h>
#include <math.h>

namespace dib {

struct AugmentDesc {
  PatchDesc p;
  float a, sigma;       // saturation factor; noise sigma in grey levels (0: none)
  unsigned key0, key1;  // Philox key of this image's noise field
};
static_assert(sizeof(AugmentDesc) == 48, "64 descriptors must stay under the kernel-argument limit");
struct AugmentBatch { AugmentDesc d[PATCH_MAX_BATCH]; };

template <typename T> __device__ __forceinline__ float quantised(T v);
// (x * 255) in the image's own dtype, truncated towards zero, clamped to 0..255, NaN -> 0: dib_deblur.hip's quantise
template <> __device__ __forceinline__ float quantised<float>(float v) {
  const float a = v * 255.0f;
  return a >= 255.0f ? 255.0f : (a > 0.0f ? truncf(a) : 0.0f);
}
template <> __device__ __forceinline__ float quantised<__half>(__half v) {
  const float a = __half2float(__float2half(__half2float(v) * 255.0f));      // the Half product is rounded to Half before the truncation
  return a >= 255.0f ? 255.0f : (a > 0.0f ? truncf(a) : 0.0f);
}

__device__ __forceinline__ float clamp255(float v) { return fminf(fmaxf(v, 0.0f), 255.0f); }

// grid (ceil(ps^2 / 256), B)
template <typename T>
__global__ __launch_bounds__(256) void patches_augment_kernel(AugmentBatch batch, int ps, float *__restrict__ out) {
#pragma clang fp contract(off)
  const AugmentDesc d = batch.d[blockIdx.y];
  const unsigned n = (unsigned)(ps * ps);
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n) return;
  const int y = (int)(e / (unsigned)ps), x = (int)(e % (unsigned)ps);
  float q[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) q[c] = quantised<T>(((const T *)d.p.in)[patch_source(d.p, ps, c, y, x)]);
  const float m = fmaxf(fmaxf(q[0], q[1]), q[2]);
  float *o = out + (size_t)blockIdx.y * 3 * n + e;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float t = d.a * (m - q[c]);
    float v = clamp255(m - t);
    if (d.sigma != 0.0f) {
      const float s = d.sigma * normal_at((unsigned long long)c * n + e, d.key0, d.key1);
      v = clamp255(v + s);
    }
    o[(size_t)c * n] = rintf(v) / 255.0f;
  }
}

}  // namespace dib

using namespace dib;

extern "C" int dib_deblur_patches_augment(const void *const *in_dev, int dtype, const int *H, const int *W, const int *py, const int *px,
                                          const unsigned int *flags, const float *saturation, const float *sigma, const unsigned int *keys,
                                          int B, int ps, float *out_dev, void *stream) {
  static const char who[] = "dib_deblur_patches_augment";
  if (dtype != DIB_F16 && dtype != DIB_F32) { set_error("%s: unknown dtype %d", who, dtype); return DIB_EINVAL; }
  if (B < 0 || B > PATCH_MAX_BATCH || ps < 1 || ps > 32768) { set_error("%s: needs 0 <= B <= %d and 1 <= ps <= 32768", who, PATCH_MAX_BATCH); return DIB_EINVAL; }
  if (B == 0) return DIB_OK;
  if (!in_dev || !H || !W || !py || !px || !flags || !saturation || !sigma || !keys || !out_dev) { set_error("%s: null pointer", who); return DIB_EINVAL; }
  if (((uintptr_t)out_dev & 3) != 0) { set_error("%s: out_dev must be 4-byte aligned", who); return DIB_EINVAL; }
  const size_t elem = dtype == DIB_F16 ? 2 : 4;
  AugmentBatch batch;
  for (int b = 0; b < B; ++b) {
    AugmentDesc &d = batch.d[b];
    const int code = patch_desc(who, b, in_dev[b], elem, H[b], W[b], py[b], px[b], flags[b], ps, &d.p);
    if (code != DIB_OK) return code;
    if (!isfinite(saturation[b]) || saturation[b] < 0.0f) {
      set_error("%s: image %d: saturation %g (needs a finite factor of at least 0)", who, b, (double)saturation[b]);
      return DIB_EINVAL;
    }
    if (!isfinite(sigma[b])) { set_error("%s: image %d: sigma %g (needs a finite noise level)", who, b, (double)sigma[b]); return DIB_EINVAL; }
    d.a = saturation[b], d.sigma = sigma[b], d.key0 = keys[2 * b], d.key1 = keys[2 * b + 1];
  }
  const dim3 grid((unsigned)(((long long)ps * ps + 255) / 256), (unsigned)B);
  if (dtype == DIB_F16) hipLaunchKernelGGL(patches_augment_kernel<__half>, grid, dim3(256), 0, (hipStream_t)stream, batch, ps, out_dev);
  else hipLaunchKernelGGL(patches_augment_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, batch, ps, out_dev);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}
