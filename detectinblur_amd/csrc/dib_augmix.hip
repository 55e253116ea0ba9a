// AugMix (reference transforms.py:68-79 around augmix/augment_and_mix.py) applied on the device to a batch of uploaded images,
// from plans the loader drew on the host (transforms.AugMix): every image gets three chains of one to three ops, each chain's
// result is normalised with the COCO mean / std and mixed,
//   mix = ((0 + ws0 N(a0)) + ws1 N(a1)) + ws2 N(a2),  out = (1 - m) N(orig) + m mix,  then * std + mean, * 255, truncated to uint8,
// all in float64 as numpy does it.  Every op of the reference works on uint8 images through Pillow, so the chains are uint8 here:
//   * point ops (autocontrast, equalize, posterize, solarize) are 256-entry LUTs per channel.  Consecutive point ops compose into one
//     LUT, built on the device from the histogram of the image they apply to (that histogram is the previous one pushed through the
//     LUT so far): a chain without positional ops never re-reads pixels.
//   * positional ops (rotate, shear, translate) are Pillow's BILINEAR affine transform (Geometry.c: affine_transform, bilinear
//     filter), one launch per positional depth; each gathers from the previous image with the pending LUT applied to its four
//     neighbours, writes a uint8 image and its histogram.
//   * the mix reads the original and each chain's last image through its final LUT and writes fp16 through the table of
//     half(float(k) / 255) (what ToTensor + .half() give the host path's uint8 result).
// Launches: histogram, LUT build, { positional stage, LUT build } per positional depth, mix.  Histograms are per-workgroup integer
// slabs summed in a fixed order by the LUT builder: no global atomics, bitwise deterministic, no host synchronisation.
// A flipped image (RandomHorizontalFlip after AugMix) is uploaded mirrored: AugMix runs in the unflipped frame by mirrored indexing of
// the input and the output; the uint8 stage images are kept unflipped.
#include "dib_common.h"

namespace dib {

constexpr int AM_THREADS = 512;   // histogram and positional stages
constexpr int AM_SLABS = 32;      // workgroups per image (or per image and chain) of the histogram kernels = histogram slabs
constexpr int AM_MIX_THREADS = 256;
constexpr int AM_LUT_THREADS = 256;
constexpr int AM_W = DIB_AUGMIX_WIDTH, AM_D = DIB_AUGMIX_MAX_DEPTH;
constexpr int HIST = 3 * 256;

__host__ __device__ inline bool am_positional(int op) {
  return op == DIB_AUGMIX_ROTATE || op == DIB_AUGMIX_SHEAR_X || op == DIB_AUGMIX_SHEAR_Y || op == DIB_AUGMIX_TRANSLATE_X ||
         op == DIB_AUGMIX_TRANSLATE_Y;
}
__host__ __device__ inline int am_positional_count(const dib_augmix_image &r, int c) {
  int p = 0;
  for (int j = 0; j < r.n_ops[c]; ++j) p += am_positional(r.op[c][j]) ? 1 : 0;
  return p;
}
// uint8 images of chain c: two (ping-pong) from its second positional op on, one for a single positional op
__host__ __device__ inline int am_buffers(const dib_augmix_image &r, int c) {
  const int p = am_positional_count(r, c);
  return p < 2 ? p : 2;
}
__host__ __device__ inline unsigned char *am_buffer(unsigned char *bufs, const dib_augmix_image &r, int c, int k) {
  long long before = 0;
  for (int j = 0; j < c; ++j) before += am_buffers(r, j);
  return bufs + r.buf_offset + (unsigned long long)(before + k) * 3ull * r.H * r.W;
}

// workspace header: hist0 slabs [n][AM_SLABS][768] u32, stage slabs [n][W][D][AM_SLABS][768] u32, LUTs [n][W][768] u8
struct AmLayout {
  size_t hist0, hists, luts, bufs;
};
inline AmLayout am_layout(int n) {
  AmLayout l;
  l.hist0 = 0;
  l.hists = l.hist0 + (size_t)n * AM_SLABS * HIST * 4;
  l.luts = l.hists + (size_t)n * AM_W * AM_D * AM_SLABS * HIST * 4;
  l.bufs = (l.luts + (size_t)n * AM_W * HIST + 255) & ~(size_t)255;
  return l;
}

// k / 255 in fp32 -> k (clamped: an input outside [0, 1] must not index past a table)
__device__ inline int am_quantize(float v) {
  const int k = (int)rintf(v * 255.f);
  return k < 0 ? 0 : (k > 255 ? 255 : k);
}

// the workgroup's LDS bins -> its slab (every bin written, empty ones as 0)
__device__ inline void am_flush_bins(const unsigned *bins, unsigned *slab) {
  for (int j = threadIdx.x; j < HIST; j += blockDim.x) slab[j] = bins[j];
}

__global__ __launch_bounds__(AM_THREADS) void augmix_hist_kernel(const dib_augmix_image *__restrict__ rec, unsigned *__restrict__ hist0) {
  __shared__ unsigned bins[HIST];
  const dib_augmix_image &r = rec[blockIdx.y];
  for (int j = threadIdx.x; j < HIST; j += blockDim.x) bins[j] = 0;
  __syncthreads();
  const int hw = r.H * r.W;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x)
    for (int c = 0; c < 3; ++c) atomicAdd(&bins[c * 256 + am_quantize(r.src[(size_t)c * hw + i])], 1u);
  __syncthreads();
  am_flush_bins(bins, hist0 + ((size_t)blockIdx.y * AM_SLABS + blockIdx.x) * HIST);
}

// Pillow ImageOps.autocontrast (cutoff 0) of one channel histogram: first and last non-empty bins lo < hi, else identity;
// entry = int(i * scale + (-lo * scale)) clamped, scale = 255.0 / (hi - lo) (a host-made table: no device division)
__device__ void am_autocontrast(const unsigned *h, unsigned char *lut, const double *scale_table) {
  int lo = 0, hi = 255;
  while (lo < 256 && h[lo] == 0) ++lo;
  while (hi >= 0 && h[hi] == 0) --hi;
  if (hi <= lo) {
    for (int i = 0; i < 256; ++i) lut[i] = (unsigned char)i;
    return;
  }
  const double scale = scale_table[hi - lo];
  const double offset = (double)(-lo) * scale;
  for (int i = 0; i < 256; ++i) {
    int v = (int)((double)i * scale + offset);
    lut[i] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
}

// Pillow ImageOps.equalize of one channel: step = (total - last non-empty bin) // 255; identity for one non-empty bin or step 0;
// else entry i = n // step, n from step // 2 growing by h[i]; entries above 255 saturate
__device__ void am_equalize(const unsigned *h, unsigned char *lut) {
  long long total = 0, last = 0;
  int nonempty = 0;
  for (int i = 0; i < 256; ++i)
    if (h[i]) { total += h[i]; last = h[i]; ++nonempty; }
  const long long step = (total - last) / 255;
  if (nonempty <= 1 || step == 0) {
    for (int i = 0; i < 256; ++i) lut[i] = (unsigned char)i;
    return;
  }
  long long n = step / 2;
  for (int i = 0; i < 256; ++i) {
    const long long v = n / step;
    lut[i] = (unsigned char)(v > 255 ? 255 : v);
    n += h[i];
  }
}

// One workgroup per (image, chain): the point ops of the chain's segment `stage` (stage 0: in front of its first positional op;
// stage s: behind its s-th) composed into one LUT per channel, starting from the identity (a positional stage bakes the LUT in
// front of it into its output).  Input histogram: the original image's (stage 0) or the s-th positional stage's, summed over slabs.
__global__ __launch_bounds__(AM_LUT_THREADS) void augmix_lut_kernel(const dib_augmix_image *__restrict__ rec, const unsigned *__restrict__ hist0,
                                                                   const unsigned *__restrict__ hists, unsigned char *__restrict__ luts,
                                                                   const double *__restrict__ scale_table, int stage) {
  __shared__ unsigned h[HIST], h2[HIST];
  __shared__ unsigned char lut[HIST], oplut[HIST];
  const int img = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
  const dib_augmix_image &r = rec[img];
  const int npos = am_positional_count(r, c);
  if (stage > npos) return;
  // the segment: ops [j0, j1)
  int j0 = 0, seen = 0;
  if (stage > 0)
    for (int j = 0; j < r.n_ops[c]; ++j)
      if (am_positional(r.op[c][j]) && ++seen == stage) { j0 = j + 1; break; }
  int j1 = j0;
  while (j1 < r.n_ops[c] && !am_positional(r.op[c][j1])) ++j1;
  const unsigned *src = stage == 0 ? hist0 + (size_t)img * AM_SLABS * HIST
                                   : hists + ((((size_t)img * AM_W + c) * AM_D + (stage - 1)) * AM_SLABS) * HIST;
  for (int k = t; k < HIST; k += blockDim.x) {
    unsigned s = 0;
    for (int b = 0; b < AM_SLABS; ++b) s += src[(size_t)b * HIST + k];   // fixed order
    h[k] = s;
    lut[k] = (unsigned char)(k & 255);
  }
  __syncthreads();
  for (int j = j0; j < j1; ++j) {
    const int op = r.op[c][j];
    if (op == DIB_AUGMIX_AUTOCONTRAST || op == DIB_AUGMIX_EQUALIZE) {
      // histogram of the image as it stands: h pushed through the LUT so far (integer adds: order-free)
      for (int k = t; k < HIST; k += blockDim.x) h2[k] = 0;
      __syncthreads();
      for (int k = t; k < HIST; k += blockDim.x)
        if (h[k]) atomicAdd(&h2[(k & ~255) + lut[k]], h[k]);
      __syncthreads();
      if (t < 3) {
        if (op == DIB_AUGMIX_AUTOCONTRAST) am_autocontrast(h2 + t * 256, oplut + t * 256, scale_table);
        else am_equalize(h2 + t * 256, oplut + t * 256);
      }
    } else {
      const int p = r.iparam[c][j];
      for (int k = t; k < HIST; k += blockDim.x) {
        const int i = k & 255;
        int v = i;
        if (op == DIB_AUGMIX_POSTERIZE) v = i & ~((1 << (8 - p)) - 1);
        else if (op == DIB_AUGMIX_SOLARIZE) v = i < p ? i : 255 - i;
        oplut[k] = (unsigned char)v;
      }
    }
    __syncthreads();
    for (int k = t; k < HIST; k += blockDim.x) lut[k] = oplut[(k & ~255) + lut[k]];
    __syncthreads();
  }
  for (int k = t; k < HIST; k += blockDim.x) luts[((size_t)img * AM_W + c) * HIST + k] = lut[k];
}

// Positional depth `depth` of every chain that has one: Pillow's BILINEAR affine (fill 0) of the previous image of the chain with
// its pending LUT applied, into a uint8 image, plus the histogram slabs of that image.  Grid: (AM_SLABS, images x chains).
__global__ __launch_bounds__(AM_THREADS) void augmix_stage_kernel(const dib_augmix_image *__restrict__ rec, unsigned char *__restrict__ bufs,
                                                                 const unsigned char *__restrict__ luts, unsigned *__restrict__ hists,
                                                                 int depth) {
  __shared__ unsigned bins[HIST];
  __shared__ unsigned char lut[HIST];
  const int img = blockIdx.y / AM_W, c = blockIdx.y % AM_W;
  const dib_augmix_image &r = rec[img];
  if (depth >= am_positional_count(r, c)) return;
  int jop = 0, seen = 0;
  for (int j = 0; j < r.n_ops[c]; ++j)
    if (am_positional(r.op[c][j]) && seen++ == depth) { jop = j; break; }
  const double *a = r.affine[c][jop];
  const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5];
  for (int k = threadIdx.x; k < HIST; k += blockDim.x) {
    bins[k] = 0;
    lut[k] = luts[((size_t)img * AM_W + c) * HIST + k];
  }
  __syncthreads();
  const int H = r.H, W = r.W, hw = H * W;
  const float *srcf = depth == 0 ? r.src : nullptr;
  const unsigned char *srcb = depth == 0 ? nullptr : am_buffer(bufs, r, c, (depth - 1) & 1);
  unsigned char *dst = am_buffer(bufs, r, c, depth & 1);
  const bool mirror = depth == 0 && r.flip;      // only the uploaded image is in the flipped frame
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
    const int y = i / W, x = i - y * W;
    const double xo = (double)x + 0.5, yo = (double)y + 0.5;
    double xin = a0 * xo + a1 * yo + a2;
    double yin = a3 * xo + a4 * yo + a5;
    int v[3] = {0, 0, 0};
    if (!(xin < 0.0 || xin >= (double)W || yin < 0.0 || yin >= (double)H)) {
      xin -= 0.5;
      yin -= 0.5;
      const int xf = (int)floor(xin), yf = (int)floor(yin);
      const double dx = xin - xf, dy = yin - yf;
      int x0 = xf < 0 ? 0 : (xf >= W ? W - 1 : xf);
      int x1 = xf + 1 < 0 ? 0 : (xf + 1 >= W ? W - 1 : xf + 1);
      const int y0 = yf < 0 ? 0 : (yf >= H ? H - 1 : yf);
      const bool second = yf + 1 >= 0 && yf + 1 < H;
      if (mirror) { x0 = W - 1 - x0; x1 = W - 1 - x1; }
      for (int ch = 0; ch < 3; ++ch) {
        const size_t plane = (size_t)ch * hw;
        int p00, p01, p10 = 0, p11 = 0;
        if (srcf) {
          p00 = am_quantize(srcf[plane + (size_t)y0 * W + x0]);
          p01 = am_quantize(srcf[plane + (size_t)y0 * W + x1]);
          if (second) {
            p10 = am_quantize(srcf[plane + (size_t)(yf + 1) * W + x0]);
            p11 = am_quantize(srcf[plane + (size_t)(yf + 1) * W + x1]);
          }
        } else {
          p00 = srcb[plane + (size_t)y0 * W + x0];
          p01 = srcb[plane + (size_t)y0 * W + x1];
          if (second) {
            p10 = srcb[plane + (size_t)(yf + 1) * W + x0];
            p11 = srcb[plane + (size_t)(yf + 1) * W + x1];
          }
        }
        const unsigned char *l = lut + ch * 256;
        const int q00 = l[p00], q01 = l[p01];
        double v1 = (double)q00 + (double)(q01 - q00) * dx;
        if (second) {
          const int q10 = l[p10], q11 = l[p11];
          const double v2 = (double)q10 + (double)(q11 - q10) * dx;
          v1 = v1 + (v2 - v1) * dy;
        }
        v[ch] = (int)v1;
      }
    }
    for (int ch = 0; ch < 3; ++ch) {
      dst[(size_t)ch * hw + i] = (unsigned char)v[ch];
      atomicAdd(&bins[ch * 256 + v[ch]], 1u);
    }
  }
  __syncthreads();
  am_flush_bins(bins, hists + ((((size_t)img * AM_W + c) * AM_D + depth) * AM_SLABS + blockIdx.x) * HIST);
}

// The mix, in the reference's float64 order, one output pixel (three channels) per lane and step.  norm: N_c[k] = (k / 255 -
// mean_c) / std_c as numpy computes it; half_table: the fp16 bits of float(k) / 255.
__global__ __launch_bounds__(AM_MIX_THREADS) void augmix_mix_kernel(const dib_augmix_image *__restrict__ rec, const unsigned char *__restrict__ bufs,
                                                                   const unsigned char *__restrict__ luts, const double *__restrict__ norm,
                                                                   const unsigned short *__restrict__ half_table) {
  __shared__ double N[HIST];
  __shared__ unsigned char lut[AM_W * HIST];
  __shared__ unsigned short h16[256];
  const int img = blockIdx.y;
  const dib_augmix_image &r = rec[img];
  for (int k = threadIdx.x; k < HIST; k += blockDim.x) N[k] = norm[k];
  for (int k = threadIdx.x; k < AM_W * HIST; k += blockDim.x) lut[k] = luts[(size_t)img * AM_W * HIST + k];
  for (int k = threadIdx.x; k < 256; k += blockDim.x) h16[k] = half_table[k];
  __syncthreads();
  const double mean[3] = {0.485, 0.456, 0.406}, stdv[3] = {0.229, 0.224, 0.225};
  const int H = r.H, W = r.W, hw = H * W;
  const unsigned char *last[AM_W];
  for (int c = 0; c < AM_W; ++c) {
    const int p = am_positional_count(r, c);
    last[c] = p ? am_buffer((unsigned char *)bufs, r, c, (p - 1) & 1) : nullptr;
  }
  const double ws[3] = {(double)r.ws[0], (double)r.ws[1], (double)r.ws[2]};
  const double m = (double)r.m, omm = (double)r.one_minus_m;
  unsigned short *dst = (unsigned short *)r.dst;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
    const int y = i / W, x = i - y * W;
    const int iu = r.flip ? y * W + (W - 1 - x) : i;     // the pixel in the unflipped frame of the stage images
    for (int ch = 0; ch < 3; ++ch) {
      const size_t plane = (size_t)ch * hw;
      const int ko = am_quantize(r.src[plane + i]);
      double mix = 0.0;
      for (int c = 0; c < AM_W; ++c) {
        const int k = last[c] ? last[c][plane + iu] : ko;
        mix = mix + ws[c] * N[ch * 256 + lut[c * HIST + ch * 256 + k]];
      }
      double o = omm * N[ch * 256 + ko] + m * mix;
      o = o * stdv[ch] + mean[ch];
      const double s = o * 255.0;
      int q = (int)s;                  // numpy's astype(uint8) of values in (-1, 256): truncation
      q = q < 0 ? 0 : (q > 255 ? 255 : q);
      dst[plane + i] = h16[q];
    }
  }
}

}  // namespace dib

using namespace dib;

extern "C" size_t dib_augmix_workspace_bytes(int n_images, unsigned long long buffer_bytes) {
  if (n_images <= 0 || n_images > 65535) return 0;
  return am_layout(n_images).bufs + (size_t)buffer_bytes;
}

extern "C" unsigned long long dib_augmix_buffer_bytes(const dib_augmix_image *plan) {
  if (!plan) return 0;
  unsigned long long n = 0;
  for (int c = 0; c < AM_W; ++c) n += (unsigned long long)am_buffers(*plan, c);
  return n * 3ull * (unsigned long long)plan->H * (unsigned long long)plan->W;
}

extern "C" int dib_augmix(const dib_augmix_image *plans_host, const dib_augmix_image *plans_dev, int n_images, const double *norm_table_dev,
                          const double *scale_table_dev, const unsigned short *half_table_dev, void *workspace_dev, size_t workspace_bytes,
                          void *stream) {
  if (n_images <= 0 || n_images > 65535 / AM_W) { set_error("dib_augmix: n_images = %d", n_images); return DIB_EINVAL; }
  if (!plans_host || !plans_dev || !norm_table_dev || !scale_table_dev || !half_table_dev || !workspace_dev) {
    set_error("dib_augmix: null pointer");
    return DIB_EINVAL;
  }
  const AmLayout l = am_layout(n_images);
  int max_hw = 1, max_pos = 0;
  for (int b = 0; b < n_images; ++b) {
    const dib_augmix_image &r = plans_host[b];
    if (!r.src || !r.dst || r.H <= 0 || r.W <= 0 || 3LL * r.H * r.W > 0x7fffffffLL) {
      set_error("dib_augmix: image %d: bad pointers or size %d x %d", b, r.H, r.W);
      return DIB_EINVAL;
    }
    for (int c = 0; c < AM_W; ++c) {
      if (r.n_ops[c] < 0 || r.n_ops[c] > AM_D) { set_error("dib_augmix: image %d chain %d: %d ops", b, c, r.n_ops[c]); return DIB_EINVAL; }
      for (int j = 0; j < r.n_ops[c]; ++j) {
        const int op = r.op[c][j], p = r.iparam[c][j];
        if (op < 0 || op > DIB_AUGMIX_TRANSLATE_Y || (op == DIB_AUGMIX_POSTERIZE && (p < 0 || p > 8)) ||
            (op == DIB_AUGMIX_SOLARIZE && (p < 0 || p > 256))) {
          set_error("dib_augmix: image %d chain %d op %d: code %d parameter %d", b, c, j, op, p);
          return DIB_EINVAL;
        }
      }
      const int p = am_positional_count(r, c);
      if (p > max_pos) max_pos = p;
    }
    if (l.bufs + r.buf_offset + dib_augmix_buffer_bytes(&r) > workspace_bytes) {
      set_error("dib_augmix: image %d: stage images end past the workspace of %zu bytes", b, workspace_bytes);
      return DIB_EINVAL;
    }
    if (r.H * r.W > max_hw) max_hw = r.H * r.W;
  }
  if (workspace_bytes < l.bufs) { set_error("dib_augmix: workspace of %zu bytes, needs at least %zu", workspace_bytes, l.bufs); return DIB_EINVAL; }
  unsigned char *ws = (unsigned char *)workspace_dev;
  unsigned *hist0 = (unsigned *)(ws + l.hist0), *hists = (unsigned *)(ws + l.hists);
  unsigned char *luts = ws + l.luts, *bufs = ws + l.bufs;
  const hipStream_t s = (hipStream_t)stream;
  const unsigned n = (unsigned)n_images;
  hipLaunchKernelGGL(augmix_hist_kernel, dim3(AM_SLABS, n), dim3(AM_THREADS), 0, s, plans_dev, hist0);
  hipLaunchKernelGGL(augmix_lut_kernel, dim3(n, AM_W), dim3(AM_LUT_THREADS), 0, s, plans_dev, hist0, hists, luts, scale_table_dev, 0);
  for (int d = 0; d < max_pos; ++d) {
    hipLaunchKernelGGL(augmix_stage_kernel, dim3(AM_SLABS, n * AM_W), dim3(AM_THREADS), 0, s, plans_dev, bufs, luts, hists, d);
    hipLaunchKernelGGL(augmix_lut_kernel, dim3(n, AM_W), dim3(AM_LUT_THREADS), 0, s, plans_dev, hist0, hists, luts, scale_table_dev, d + 1);
  }
  long long blocks = (max_hw + AM_MIX_THREADS - 1) / AM_MIX_THREADS;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(augmix_mix_kernel, dim3((unsigned)blocks, n), dim3(AM_MIX_THREADS), 0, s, plans_dev, bufs, luts, norm_table_dev,
                     half_table_dev);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}
