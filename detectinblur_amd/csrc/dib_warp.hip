// "Squint" warp (`--warp_in_model`, reference models/warper.py:47-50) on fp32 activations: the reference's Half affine_grid and its
// bilinear grid_sample (zeros outside, align_corners False) in ONE launch -- no grid tensor, no Half copy of the input.  The
// arithmetic is the one include/dib.h states (and models/warper.py: squint_half_grid restates in torch):
//   gx = half((m00 * bx + m01 * by) + m02),  gy = half((m10 * bx + m11 * by) + m12)     fp32 sums of exact products, one rounding to Half
//   ix = ((gx + 1) * W - 1) / 2,             iy = ((gy + 1) * H - 1) / 2                fp32
// and the four corners around (ix, iy), each with torch's weight expression.  A corner inside the image is always multiplied and
// added (weight 0 times NaN is NaN, as in torch); a corner outside is skipped.
//
// Work split: a workgroup serves (part of) ONE image row, so the matrix and the row's `by` are workgroup-uniform.
//   forward, channels-last, C % 4 == 0: a lane = 4 channels of one pixel (16-byte loads and stores); at C = 256 a wave is one pixel
//   forward, anything else (the image's C = 3, planar tensors): a lane = one pixel, looping over the channels
//   backward: a lane = ONE float of grad_out, so that a wave's atomic instruction covers contiguous channels of one corner
//             (channels-last: 256 contiguous bytes at C >= 64, the shape float atomics run at full rate in)
#include <hip/hip_fp16.h>

#include "dib_common.h"

namespace dib {

struct WarpGeom {
  int N, C, H, W;
  long long sN, sC, sY, sX;      // element strides of (n, c, i, j)
};

struct WarpTaps {
  int x0, y0;                    // north-west corner, clamped to [-1, W] x [-1, H] (only read where the flags say "inside")
  bool x0_in, x1_in, y0_in, y1_in;
  float nw, ne, sw, se;
};

__device__ __forceinline__ float half_bits_to_float(unsigned short b) { return __half2float(__ushort_as_half(b)); }
__device__ __forceinline__ float round_to_half(float v) { return __half2float(__float2half_rn(v)); }

// m: the image's six Half matrix entries; bx, by: the pixel's base coordinates (already fp32)
__device__ __forceinline__ WarpTaps warp_taps(const unsigned short *__restrict__ m, float bx, float by, int H, int W) {
  const float m00 = half_bits_to_float(m[0]), m01 = half_bits_to_float(m[1]), m02 = half_bits_to_float(m[2]);
  const float m10 = half_bits_to_float(m[3]), m11 = half_bits_to_float(m[4]), m12 = half_bits_to_float(m[5]);
  const float gx = round_to_half((m00 * bx + m01 * by) + m02);
  const float gy = round_to_half((m10 * bx + m11 * by) + m12);
  const float ix = ((gx + 1.f) * (float)W - 1.f) / 2.f;
  const float iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
  const float fx = floorf(ix), fy = floorf(iy);
  const float lx = ix - fx, hx = (fx + 1.f) - ix, ly = iy - fy, hy = (fy + 1.f) - iy;
  WarpTaps t;
  // compared as floats: a NaN or infinite coordinate (a diverged matrix) is inside nowhere and never becomes an index
  t.x0_in = fx >= 0.f && fx <= (float)(W - 1);
  t.x1_in = fx >= -1.f && fx <= (float)(W - 2);
  t.y0_in = fy >= 0.f && fy <= (float)(H - 1);
  t.y1_in = fy >= -1.f && fy <= (float)(H - 2);
  t.x0 = (int)fminf(fmaxf(fx, -1.f), (float)W);
  t.y0 = (int)fminf(fmaxf(fy, -1.f), (float)H);
  t.nw = hx * hy; t.ne = lx * hy; t.sw = hx * ly; t.se = lx * ly;
  return t;
}

__device__ __forceinline__ void madd4(float4 &a, float w, const float4 v) {
  a.x += w * v.x; a.y += w * v.y; a.z += w * v.z; a.w += w * v.w;
}

// grid: x = image row (n * H + i), y = chunks of 256 lanes over the row's W * C4 (pixel, channel quad) pairs
__global__ __launch_bounds__(256) void squint_fwd_nhwc4_kernel(const float4 *__restrict__ in, float4 *__restrict__ out, int H, int W, int C4,
                                                               const unsigned short *__restrict__ mats, const unsigned short *__restrict__ base_x,
                                                               const unsigned short *__restrict__ base_y) {
  const int row = blockIdx.x, n = row / H, i = row - n * H;
  const int t = blockIdx.y * 256 + threadIdx.x;
  if (t >= W * C4) return;
  const int j = t / C4, q = t - j * C4;
  const WarpTaps p = warp_taps(mats + (size_t)n * 6, half_bits_to_float(base_x[j]), half_bits_to_float(base_y[i]), H, W);
  const float4 *img = in + (size_t)n * H * W * C4 + q;
  // all four loads are issued before the first use: a corner outside the image reads the nearest pixel inside (never used)
  const size_t xa = (size_t)min(max(p.x0, 0), W - 1) * C4, xb = (size_t)min(max(p.x0 + 1, 0), W - 1) * C4;
  const float4 *ra = img + (size_t)min(max(p.y0, 0), H - 1) * W * C4, *rb = img + (size_t)min(max(p.y0 + 1, 0), H - 1) * W * C4;
  const float4 v00 = ra[xa], v01 = ra[xb], v10 = rb[xa], v11 = rb[xb];
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (p.y0_in && p.x0_in) madd4(acc, p.nw, v00);
  if (p.y0_in && p.x1_in) madd4(acc, p.ne, v01);
  if (p.y1_in && p.x0_in) madd4(acc, p.sw, v10);
  if (p.y1_in && p.x1_in) madd4(acc, p.se, v11);
  out[((size_t)row * W + j) * C4 + q] = acc;
}

// grid: x = image row (n * H + i), y = chunks of 64 pixels of the row; any strides
__global__ __launch_bounds__(64) void squint_fwd_scalar_kernel(const float *__restrict__ in, float *__restrict__ out, WarpGeom g,
                                                               const unsigned short *__restrict__ mats, const unsigned short *__restrict__ base_x,
                                                               const unsigned short *__restrict__ base_y) {
  const int row = blockIdx.x, n = row / g.H, i = row - n * g.H;
  const int j = blockIdx.y * 64 + threadIdx.x;
  if (j >= g.W) return;
  const WarpTaps p = warp_taps(mats + (size_t)n * 6, half_bits_to_float(base_x[j]), half_bits_to_float(base_y[i]), g.H, g.W);
  const float *img = in + n * g.sN;
  float *dst = out + n * g.sN + i * g.sY + j * g.sX;
  // as above: clamped addresses, four loads in flight per channel
  const long long xa = min(max(p.x0, 0), g.W - 1) * g.sX, xb = min(max(p.x0 + 1, 0), g.W - 1) * g.sX;
  const long long ya = min(max(p.y0, 0), g.H - 1) * g.sY, yb = min(max(p.y0 + 1, 0), g.H - 1) * g.sY;
  const long long o00 = ya + xa, o01 = ya + xb, o10 = yb + xa, o11 = yb + xb;
  for (int c = 0; c < g.C; ++c) {
    const float *pl = img + c * g.sC;
    const float v00 = pl[o00], v01 = pl[o01], v10 = pl[o10], v11 = pl[o11];
    float acc = 0.f;
    if (p.y0_in && p.x0_in) acc += p.nw * v00;
    if (p.y0_in && p.x1_in) acc += p.ne * v01;
    if (p.y1_in && p.x0_in) acc += p.sw * v10;
    if (p.y1_in && p.x1_in) acc += p.se * v11;
    dst[c * g.sC] = acc;
  }
}

// One lane per float of grad_out.  grid x = a row of grad_out, y = chunks of 256 lanes over it:
//   NHWC:   row = n * H + i,            lane t = (j, c) with c fastest: a wave adds to contiguous channels of one corner
//   planar: row = (n * C + c) * H + i,  lane t = j
template <bool NHWC>
__global__ __launch_bounds__(256) void squint_bwd_kernel(const float *__restrict__ gout, float *__restrict__ gin, WarpGeom g,
                                                         const unsigned short *__restrict__ mats, const unsigned short *__restrict__ base_x,
                                                         const unsigned short *__restrict__ base_y) {
  const int row = blockIdx.x, t = blockIdx.y * 256 + threadIdx.x;
  int n, c, i, j;
  if (NHWC) {
    if (t >= g.W * g.C) return;
    n = row / g.H; i = row - n * g.H;
    j = t / g.C; c = t - j * g.C;
  } else {
    if (t >= g.W) return;
    const int nc = row / g.H;
    i = row - nc * g.H;
    n = nc / g.C; c = nc - n * g.C;
    j = t;
  }
  const WarpTaps p = warp_taps(mats + (size_t)n * 6, half_bits_to_float(base_x[j]), half_bits_to_float(base_y[i]), g.H, g.W);
  const long long plane = n * g.sN + c * g.sC;
  const float go = gout[plane + i * g.sY + j * g.sX];
  float *r = gin + plane + p.y0 * g.sY + p.x0 * g.sX;
  if (p.y0_in && p.x0_in) atomicAdd(r, p.nw * go);
  if (p.y0_in && p.x1_in) atomicAdd(r + g.sX, p.ne * go);
  if (p.y1_in && p.x0_in) atomicAdd(r + g.sY, p.sw * go);
  if (p.y1_in && p.x1_in) atomicAdd(r + g.sY + g.sX, p.se * go);
}

static int warp_check(const char *who, const void *a, const void *b, int N, int C, int H, int W, int layout, const void *mats, const void *bx,
                      const void *by, WarpGeom *g) {
  if (!a || !b || !mats || !bx || !by) { set_error("%s: null pointer", who); return DIB_EINVAL; }
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) { set_error("%s: needs N, C, H, W > 0 (got %d, %d, %d, %d)", who, N, C, H, W); return DIB_EINVAL; }
  if (layout != DIB_WARP_NHWC && layout != DIB_WARP_NCHW) { set_error("%s: unknown layout %d", who, layout); return DIB_EINVAL; }
  // grid x carries a row index ((n, i), or (n, c, i) in the planar backward pass), grid y chunks of a row's W * C lanes
  if ((long long)N * C * H > 0x7fffffffLL || (long long)W * C > 65535LL * 256) {
    set_error("%s: N * C * H = %lld or W * C = %lld too large for one launch", who, (long long)N * C * H, (long long)W * C);
    return DIB_EINVAL;
  }
  g->N = N; g->C = C; g->H = H; g->W = W;
  g->sN = (long long)C * H * W;
  if (layout == DIB_WARP_NHWC) { g->sC = 1; g->sX = C; g->sY = (long long)W * C; }
  else { g->sC = (long long)H * W; g->sX = 1; g->sY = W; }
  return DIB_OK;
}

}  // namespace dib

using namespace dib;

extern "C" int dib_squint_warp_forward(const float *in_dev, float *out_dev, int N, int C, int H, int W, int layout, const unsigned short *mats_dev,
                                       const unsigned short *base_x_dev, const unsigned short *base_y_dev, void *stream) {
  WarpGeom g;
  const int rc = warp_check("dib_squint_warp_forward", in_dev, out_dev, N, C, H, W, layout, mats_dev, base_x_dev, base_y_dev, &g);
  if (rc != DIB_OK) return rc;
  if (in_dev == out_dev) { set_error("dib_squint_warp_forward: out must not alias in"); return DIB_EINVAL; }
  const hipStream_t s = (hipStream_t)stream;
  const unsigned rows = (unsigned)(N * H);
  if (layout == DIB_WARP_NHWC && (C % 4) == 0 && (((uintptr_t)in_dev | (uintptr_t)out_dev) & 15) == 0) {
    const int C4 = C / 4;
    hipLaunchKernelGGL(squint_fwd_nhwc4_kernel, dim3(rows, (unsigned)((W * C4 + 255) / 256)), dim3(256), 0, s, (const float4 *)in_dev,
                       (float4 *)out_dev, H, W, C4, mats_dev, base_x_dev, base_y_dev);
  } else {
    hipLaunchKernelGGL(squint_fwd_scalar_kernel, dim3(rows, (unsigned)((W + 63) / 64)), dim3(64), 0, s, in_dev, out_dev, g, mats_dev,
                       base_x_dev, base_y_dev);
  }
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

extern "C" int dib_squint_warp_backward(const float *grad_out_dev, float *grad_in_dev, int N, int C, int H, int W, int layout,
                                        const unsigned short *mats_dev, const unsigned short *base_x_dev, const unsigned short *base_y_dev,
                                        void *stream) {
  WarpGeom g;
  const int rc = warp_check("dib_squint_warp_backward", grad_out_dev, grad_in_dev, N, C, H, W, layout, mats_dev, base_x_dev, base_y_dev, &g);
  if (rc != DIB_OK) return rc;
  if (grad_out_dev == grad_in_dev) { set_error("dib_squint_warp_backward: grad_in must not alias grad_out"); return DIB_EINVAL; }
  const hipStream_t s = (hipStream_t)stream;
  if (layout == DIB_WARP_NHWC)
    hipLaunchKernelGGL(squint_bwd_kernel<true>, dim3((unsigned)(N * H), (unsigned)((W * C + 255) / 256)), dim3(256), 0, s, grad_out_dev,
                       grad_in_dev, g, mats_dev, base_x_dev, base_y_dev);
  else
    hipLaunchKernelGGL(squint_bwd_kernel<false>, dim3((unsigned)(N * C * H), (unsigned)((W + 255) / 256)), dim3(256), 0, s, grad_out_dev,
                       grad_in_dev, g, mats_dev, base_x_dev, base_y_dev);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}
