// Test-time batch-norm statistics ("mode one", reference models/batchnorm.py:159-184) for channels-last (NHWC) fp32
// activations of the ResNet-50 trunk: every batch-norm layer normalises with its running statistics mixed with the
// statistics of the batch it sees,
//   mean = f * running_mean + g * mean_b,  var = f * running_var + g * var_b,  f = n / (n + 1), g = 1 / (n + 1),
// then y = act(x * scale[c] + shift[c] (+ residual)) with scale = w / sqrt(var + eps), shift = b - mean * scale.
//
// Three launches, no atomics, no host synchronisation (graph-capturable):
//   1. bn_partial_kernel: workgroup (slice s, channel chunk k).  Each lane owns 4 consecutive channels (float4 loads: a
//      wave reads 1 KiB of a pixel row when C >= 256) and every R-th pixel of the slice, and keeps (count, mean, M2) per
//      channel with Welford's update -- never sum(x^2) - sum(x)^2 / n, which loses every digit for |mean| >> std.  The R
//      pixel rows of the workgroup are merged in LDS with Chan's formula in a fixed tree order; one (mean, M2) per channel
//      per slice goes to the workspace.
//   2. bn_finalize_kernel: 64 channels per workgroup, 16 lanes per channel merge the slices (lane j: slices j, j + 16, ...,
//      in order), the 16 partial results merge in lane order; then the mix above and scale / shift.
//   3. bn_apply_kernel: the in-place pass of bias_act_kernel (dib_eltwise_vec.h) with a scale.
// Every reduction runs in an order fixed by the shape alone: two calls on the same input are bitwise equal.
//
// Acclimation (reference models/batchnorm.py:142-157, dib_bn_acclimate_nhwc) is the online form of the same remedy, in the same
// three launches: bn_acclimate_finalize_kernel folds the batch's mean and UNBIASED variance into the running statistics with
// factor a (the momentum, or 1 / num_batches_tracked after its bump), writes them back and normalises with the updated pair;
// the bumped counter is stored by the apply launch (bn_apply_bump_kernel), behind every read of the old value.
//
// Host side: both entry points refuse what only they can be given wrong and then call bn_run, which holds the refusals they
// share, the geometry, the workspace layout (bn_workspace, also behind the size query) and the three launches; an entry point
// supplies its finalize launch and says whether the apply launch bumps the counter.
#include "dib_eltwise_vec.h"      // host side only: misaligned, grid_1d, launch

namespace dib {

constexpr int BN_THREADS = 1024;     // partial statistics: 16 waves per workgroup
constexpr int BN_MAX_SLICES = 256;
constexpr int BN_FIN_LANES = 16;     // finalize: lanes per channel (a workgroup: 64 channels x 16 lanes)
constexpr int BN_FIN_BATCH = 4;      // slices a finalize lane loads before merging them (16 spill at 1,024 lanes per workgroup)

struct Welford {
  float n, mean, m2;
};

// Chan et al.: merge b into a.  Each product and sum rounded separately (the library builds with -ffp-contract=off).
__device__ inline void chan_merge(Welford &a, const Welford &b) {
  if (b.n == 0.f) return;
  if (a.n == 0.f) { a = b; return; }
  const float n = a.n + b.n;
  const float d = b.mean - a.mean;
  const float wb = b.n / n;
  a.mean = a.mean + d * wb;
  a.m2 = a.m2 + b.m2 + d * d * (a.n * wb);
  a.n = n;
}

struct BnGeom {
  long long npix;   // N * H * W
  int C, Q;         // channels, channel quads
  int QB, R;        // quads per workgroup, pixel rows per workgroup (QB * R <= BN_THREADS)
  int S;            // pixel slices
};

__host__ __device__ inline long long slice_begin(long long npix, int S, int s) { return npix * s / S; }

__global__ __launch_bounds__(BN_THREADS) void bn_partial_kernel(const float4 *__restrict__ x, BnGeom g, float *__restrict__ ws_mean,
                                                                float *__restrict__ ws_m2) {
  __shared__ float4 sh_mean[BN_THREADS], sh_m2[BN_THREADS];
  __shared__ float sh_n[BN_THREADS];
  const int t = threadIdx.x;
  const int qi = t % g.QB, row = t / g.QB;
  const int q = blockIdx.y * g.QB + qi;
  const int s = blockIdx.x;
  const bool active = row < g.R && q < g.Q;
  const long long p0 = slice_begin(g.npix, g.S, s), p1 = slice_begin(g.npix, g.S, s + 1);
  float n = 0.f;
  float4 mean = make_float4(0.f, 0.f, 0.f, 0.f), m2 = mean;
  if (active) {
    const float4 *src = x + q;
    long long p = p0 + row;
    // four loads in flight per lane, then four Welford updates in pixel order
    for (; p + 3LL * g.R < p1; p += 4LL * g.R) {
      float4 v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = src[(p + (long long)k * g.R) * g.Q];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        n += 1.f;
        const float r = 1.f / n;
        float d;
        d = v[k].x - mean.x; mean.x = mean.x + d * r; m2.x = m2.x + d * (v[k].x - mean.x);
        d = v[k].y - mean.y; mean.y = mean.y + d * r; m2.y = m2.y + d * (v[k].y - mean.y);
        d = v[k].z - mean.z; mean.z = mean.z + d * r; m2.z = m2.z + d * (v[k].z - mean.z);
        d = v[k].w - mean.w; mean.w = mean.w + d * r; m2.w = m2.w + d * (v[k].w - mean.w);
      }
    }
    for (; p < p1; p += g.R) {
      const float4 v = src[p * g.Q];
      n += 1.f;
      const float r = 1.f / n;
      float d;
      d = v.x - mean.x; mean.x = mean.x + d * r; m2.x = m2.x + d * (v.x - mean.x);
      d = v.y - mean.y; mean.y = mean.y + d * r; m2.y = m2.y + d * (v.y - mean.y);
      d = v.z - mean.z; mean.z = mean.z + d * r; m2.z = m2.z + d * (v.z - mean.z);
      d = v.w - mean.w; mean.w = mean.w + d * r; m2.w = m2.w + d * (v.w - mean.w);
    }
  }
  sh_mean[t] = mean;
  sh_m2[t] = m2;
  sh_n[t] = n;
  __syncthreads();
  // tree over the rows in a fixed order: row r takes row r + h (any R, not only powers of two)
  int h = 1;
  while (h < g.R) h <<= 1;
  for (h >>= 1; h >= 1; h >>= 1) {
    if (active && row < h && row + h < g.R) {
      const int u = t + h * g.QB;
      Welford a, b;
      const float4 am = sh_mean[t], a2 = sh_m2[t], bm = sh_mean[u], b2 = sh_m2[u];
      float4 om, o2;
      a = {sh_n[t], am.x, a2.x}; b = {sh_n[u], bm.x, b2.x}; chan_merge(a, b); om.x = a.mean; o2.x = a.m2;
      a = {sh_n[t], am.y, a2.y}; b = {sh_n[u], bm.y, b2.y}; chan_merge(a, b); om.y = a.mean; o2.y = a.m2;
      a = {sh_n[t], am.z, a2.z}; b = {sh_n[u], bm.z, b2.z}; chan_merge(a, b); om.z = a.mean; o2.z = a.m2;
      a = {sh_n[t], am.w, a2.w}; b = {sh_n[u], bm.w, b2.w}; chan_merge(a, b); om.w = a.mean; o2.w = a.m2;
      sh_mean[t] = om;
      sh_m2[t] = o2;
      sh_n[t] = a.n;
    }
    __syncthreads();
  }
  if (active && row == 0) {
    reinterpret_cast<float4 *>(ws_mean + (long long)s * g.C)[q] = sh_mean[t];
    reinterpret_cast<float4 *>(ws_m2 + (long long)s * g.C)[q] = sh_m2[t];
  }
}

// The slices of one channel merged by BN_FIN_LANES lanes (lane j: slices j, j + 16, ..., in order), then the 16 partial results
// in lane order.  Every lane of the workgroup calls this (it holds a barrier); true on the one lane per channel (j == 0) that
// leaves with the channel's (count, mean, M2) in `acc`.  Both finalize kernels call it: the merge order is stated once.
__device__ inline bool bn_merge_slices(const BnGeom &g, const float *__restrict__ ws_mean, const float *__restrict__ ws_m2,
                                       float (*sh)[BN_FIN_LANES][64], int c, Welford &acc) {
  const int cl = threadIdx.x & 63, j = threadIdx.x >> 6;
  acc = {0.f, 0.f, 0.f};
  if (c < g.C) {
    // BN_FIN_BATCH slices' loads in flight, then their merges in slice order: the partial results were just written by workgroups
    // on other XCDs, and load round trips, not bandwidth, are this kernel's cost (7-15 us per layer: profiles/mode_one_norm.txt)
    for (int s0 = j; s0 < g.S; s0 += BN_FIN_BATCH * BN_FIN_LANES) {
      float m[BN_FIN_BATCH], q[BN_FIN_BATCH];
#pragma unroll
      for (int k = 0; k < BN_FIN_BATCH; ++k) {
        const int s = s0 + k * BN_FIN_LANES;
        m[k] = s < g.S ? ws_mean[(long long)s * g.C + c] : 0.f;
        q[k] = s < g.S ? ws_m2[(long long)s * g.C + c] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < BN_FIN_BATCH; ++k) {
        const int s = s0 + k * BN_FIN_LANES;
        if (s < g.S) chan_merge(acc, Welford{(float)(slice_begin(g.npix, g.S, s + 1) - slice_begin(g.npix, g.S, s)), m[k], q[k]});
      }
    }
  }
  sh[0][j][cl] = acc.n;
  sh[1][j][cl] = acc.mean;
  sh[2][j][cl] = acc.m2;
  __syncthreads();
  if (j != 0 || c >= g.C) return false;
  for (int k = 1; k < BN_FIN_LANES; ++k) chan_merge(acc, Welford{sh[0][k][cl], sh[1][k][cl], sh[2][k][cl]});
  return true;
}

__global__ __launch_bounds__(64 * BN_FIN_LANES) void bn_finalize_kernel(BnGeom g, const float *__restrict__ ws_mean, const float *__restrict__ ws_m2,
                                                          const float *__restrict__ weight, const float *__restrict__ bias,
                                                          const float *__restrict__ running_mean, const float *__restrict__ running_var,
                                                          const long long *__restrict__ nbt_dev, long long nbt_host, float eps,
                                                          float *__restrict__ scale, float *__restrict__ shift,
                                                          float *__restrict__ stats) {
  __shared__ float sh[3][BN_FIN_LANES][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  Welford acc;
  if (!bn_merge_slices(g, ws_mean, ws_m2, sh, c, acc)) return;
  // the reference's factors: torch.true_divide of int64 tensors, i.e. float32(n) / float32(n + 1) and 1 / float32(n + 1)
  const long long nb = nbt_dev ? *nbt_dev : nbt_host;
  const float f = (float)nb / (float)(nb + 1);
  const float gg = 1.f / (float)(nb + 1);
  const float var_b = acc.m2 / acc.n;              // biased: var(unbiased=False)
  const float fm = f * running_mean[c], gm = gg * acc.mean;
  const float fv = f * running_var[c], gv = gg * var_b;
  const float mean = fm + gm, var = fv + gv;
  const float sc = (weight ? weight[c] : 1.f) * (1.f / sqrtf(var + eps));
  scale[c] = sc;
  shift[c] = (bias ? bias[c] : 0.f) - mean * sc;
  if (stats) {
    stats[c] = mean;
    stats[g.C + c] = var;
  }
}

// Acclimation (reference models/batchnorm.py:142-157): the batch's statistics are folded into the running ones, which are written
// back, and the layer normalises with the UPDATED running statistics.  One lane per channel reads and writes that channel's
// running pair.  The counter is only READ here, by every workgroup: its bumped value is stored by the apply launch
// (bn_apply_bump_kernel), which the stream orders behind all of these reads.
__global__ __launch_bounds__(64 * BN_FIN_LANES) void bn_acclimate_finalize_kernel(BnGeom g, const float *__restrict__ ws_mean,
                                                          const float *__restrict__ ws_m2, const float *__restrict__ weight,
                                                          const float *__restrict__ bias, float *__restrict__ running_mean,
                                                          float *__restrict__ running_var, const long long *__restrict__ nbt_dev,
                                                          int bump, float momentum, float eps, float *__restrict__ scale,
                                                          float *__restrict__ shift, float *__restrict__ stats) {
  __shared__ float sh[3][BN_FIN_LANES][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  // the lane that will hold the channel's statistics asks for everything else it needs BEFORE the merge, so that these loads and
  // the division travel under the merge's own load round trips instead of behind them (profiles/acclimate_norm.txt).
  // a is the reference's exponential_average_factor (:110-122): the momentum, or 1 / float(num_batches_tracked) AFTER the bump (python
  // floats: the division in double, rounded once to the float that ATen's fp32 update takes); without a bump and without a
  // momentum it stays 0.0
  float a = momentum, rm = 0.f, rv = 1.f, w = 1.f, b = 0.f;
  if ((threadIdx.x >> 6) == 0 && c < g.C) {
    if (momentum < 0.f) a = bump ? (float)(1.0 / (double)(*nbt_dev + 1)) : 0.f;
    rm = running_mean[c];
    rv = running_var[c];
    if (weight) w = weight[c];
    if (bias) b = bias[c];
  }
  Welford acc;
  if (!bn_merge_slices(g, ws_mean, ws_m2, sh, c, acc)) return;
  const float keep = 1.f - a;
  const float var_u = acc.m2 / (acc.n - 1.f);      // unbiased: what training-mode batch_norm folds into running_var
  const float km = keep * rm, am = a * acc.mean;
  const float kv = keep * rv, av = a * var_u;
  const float mean = km + am, var = kv + av;
  running_mean[c] = mean;
  running_var[c] = var;
  const float sc = w * (1.f / sqrtf(var + eps));
  scale[c] = sc;
  shift[c] = b - mean * sc;
  if (stats) {
    stats[c] = acc.mean;
    stats[g.C + c] = var_u;
    stats[2 * g.C + c] = mean;
    stats[3 * g.C + c] = var;
  }
}

template <bool RES, bool RELU>
__device__ inline void bn_apply_body(float4 *__restrict__ x, const float4 *__restrict__ scale, const float4 *__restrict__ shift,
                                     const float4 *__restrict__ res, long long n4, int C4) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 v = x[i];
    const int c = (int)(i % C4);
    const float4 a = scale[c], b = shift[c];
    v.x = v.x * a.x + b.x; v.y = v.y * a.y + b.y; v.z = v.z * a.z + b.z; v.w = v.w * a.w + b.w;
    if (RES) { const float4 r = res[i]; v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w; }
    if (RELU) { v.x = relu_keep_nan(v.x); v.y = relu_keep_nan(v.y); v.z = relu_keep_nan(v.z); v.w = relu_keep_nan(v.w); }
    x[i] = v;
  }
}

template <bool RES, bool RELU>
__global__ __launch_bounds__(256) void bn_apply_kernel(float4 *__restrict__ x, const float4 *__restrict__ scale,
                                                       const float4 *__restrict__ shift, const float4 *__restrict__ res, long long n4,
                                                       int C4) {
  bn_apply_body<RES, RELU>(x, scale, shift, res, n4, C4);
}

// the apply pass of an acclimating layer in training mode: one lane also stores num_batches_tracked + 1.  Nothing in this launch
// reads the counter but that lane, and every reader of the old value (bn_acclimate_finalize_kernel) ran in the launch before.
template <bool RES, bool RELU>
__global__ __launch_bounds__(256) void bn_apply_bump_kernel(float4 *__restrict__ x, const float4 *__restrict__ scale,
                                                            const float4 *__restrict__ shift, const float4 *__restrict__ res,
                                                            long long n4, int C4, long long *__restrict__ nbt) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *nbt = *nbt + 1;
  bn_apply_body<RES, RELU>(x, scale, shift, res, n4, C4);
}

// Grid of the partial statistics: up to 64 quads (256 channels) side by side, as many pixel rows as fill BN_THREADS lanes,
// and enough slices for ~1,000 workgroups (4 per CU) while every lane keeps at least 4 pixels.  Batch 1 at 800 x 1344:
// layer1 (67,200 px x 256 ch): 256 slices x 1 chunk, 16 rows, ~16 px per lane; layer4 (1,050 px x 2,048 ch): 16 slices x 8
// chunks, 16 rows, ~4 px per lane; the stem (268,800 px x 64 ch): 256 slices, 64 rows, ~16 px per lane.
static BnGeom bn_geometry(long long npix, int C) {
  BnGeom g;
  g.npix = npix;
  g.C = C;
  g.Q = C / 4;
  g.QB = g.Q < 64 ? g.Q : 64;
  g.R = BN_THREADS / g.QB;
  const long long chunks = (g.Q + g.QB - 1) / g.QB;
  long long S = (1024 + chunks - 1) / chunks;
  const long long by_pixels = npix / (4LL * g.R);
  if (S > by_pixels) S = by_pixels;
  if (S > BN_MAX_SLICES) S = BN_MAX_SLICES;
  if (S < 1) S = 1;
  g.S = (int)S;
  return g;
}

// The workspace layout, stated once: scale [C], shift [C], slice means [S][C], slice M2 [S][C] (floats).  The size query calls
// this with a null base and reads only `floats`.
struct BnWorkspace {
  float *scale, *shift, *ws_mean, *ws_m2;
  size_t floats;
};

static BnWorkspace bn_workspace(const BnGeom &g, void *base) {
  const size_t C = (size_t)g.C, slices = (size_t)g.S * C;
  float *ws = (float *)base;
  return {ws, ws + C, ws + 2 * C, ws + 2 * C + slices, 2 * C + 2 * slices};
}

template <bool RES, bool RELU>
static int bn_apply(float *x, const BnWorkspace &w, const float *res, long long n4, int C4, long long *bump_nbt, void *stream) {
  // grid_1d caps the grid at 2^30 workgroups; both kernels stride over what is left, which takes more than 2^38 elements
  if (bump_nbt) return launch(bn_apply_bump_kernel<RES, RELU>, grid_1d(n4), stream, x, w.scale, w.shift, res, n4, C4, bump_nbt);
  return launch(bn_apply_kernel<RES, RELU>, grid_1d(n4), stream, x, w.scale, w.shift, res, n4, C4);
}

// The host sequence of both entry points (`who`): the refusals they share, then the three launches on `stream`.
//   align_rule   the entry point's sentence about alignment (acclimation's names its counter as well)
//   finalize     (grid, block, stream, g, workspace) -> launches the entry point's finalize kernel
//   bump_nbt     the counter that the apply launch bumps (bn_apply_bump_kernel), or null (bn_apply_kernel)
template <class Finalize>
static int bn_run(const char *who, const char *align_rule, float *x_dev, const float *residual_dev, long long n_pix, int C,
                  const float *running_mean_dev, const float *running_var_dev, int relu, long long *bump_nbt, void *workspace_dev,
                  size_t workspace_bytes, void *stream, Finalize finalize) {
  if (n_pix <= 0 || C <= 0 || (C % 4) != 0 || C / 4 > 65535LL * 64) { set_error("%s: needs n_pix > 0 and C %% 4 == 0 (C = %d)", who, C); return DIB_EINVAL; }
  if (!x_dev || !running_mean_dev || !running_var_dev || !workspace_dev) { set_error("%s: null pointer", who); return DIB_EINVAL; }
  if (misaligned({x_dev, residual_dev, workspace_dev})) { set_error("%s: %s", who, align_rule); return DIB_EINVAL; }
  const BnGeom g = bn_geometry(n_pix, C);
  const BnWorkspace w = bn_workspace(g, workspace_dev);
  const size_t need = w.floats * sizeof(float);
  if (workspace_bytes < need) { set_error("%s: workspace of %zu bytes, needs %zu", who, workspace_bytes, need); return DIB_EINVAL; }
  const hipStream_t s = (hipStream_t)stream;
  const unsigned chunks = (unsigned)((g.Q + g.QB - 1) / g.QB);
  hipLaunchKernelGGL(bn_partial_kernel, dim3((unsigned)g.S, chunks), dim3(BN_THREADS), 0, s, (const float4 *)x_dev, g, w.ws_mean, w.ws_m2);
  finalize(dim3((unsigned)((C + 63) / 64)), dim3(64 * BN_FIN_LANES), s, g, w);
  const auto apply = residual_dev ? (relu ? bn_apply<true, true> : bn_apply<true, false>)
                                  : (relu ? bn_apply<false, true> : bn_apply<false, false>);
  return apply(x_dev, w, residual_dev, n_pix * (C / 4), C / 4, bump_nbt, stream);      // one float4 per lane
}

}  // namespace dib

using namespace dib;

extern "C" size_t dib_bn_mode_one_workspace_bytes(long long n_pix, int C) {
  if (n_pix <= 0 || C <= 0 || (C % 4) != 0) return 0;
  return bn_workspace(bn_geometry(n_pix, C), nullptr).floats * sizeof(float);
}

extern "C" int dib_bn_mode_one_nhwc(float *x_dev, const float *residual_dev, long long n_pix, int C, const float *weight_dev,
                                    const float *bias_dev, const float *running_mean_dev, const float *running_var_dev,
                                    const long long *num_batches_dev, long long num_batches, float eps, int relu, void *workspace_dev,
                                    size_t workspace_bytes, float *stats_dev, void *stream) {
  static const char who[] = "dib_bn_mode_one_nhwc";
  if (!num_batches_dev && num_batches < 0) { set_error("%s: negative num_batches_tracked", who); return DIB_EINVAL; }
  return bn_run(who, "x, residual and workspace must be 16-byte aligned", x_dev, residual_dev, n_pix, C, running_mean_dev, running_var_dev,
                relu, nullptr, workspace_dev, workspace_bytes, stream,
                [&](dim3 grid, dim3 block, hipStream_t s, const BnGeom &g, const BnWorkspace &w) {
                  hipLaunchKernelGGL(bn_finalize_kernel, grid, block, 0, s, g, w.ws_mean, w.ws_m2, weight_dev, bias_dev, running_mean_dev,
                                     running_var_dev, num_batches_dev, num_batches, eps, w.scale, w.shift, stats_dev);
                });
}

extern "C" int dib_bn_acclimate_nhwc(float *x_dev, const float *residual_dev, long long n_pix, int C, const float *weight_dev,
                                     const float *bias_dev, float *running_mean_dev, float *running_var_dev, long long *num_batches_dev,
                                     int bump, float momentum, float eps, int relu, void *workspace_dev, size_t workspace_bytes,
                                     float *stats_dev, void *stream) {
  static const char who[] = "dib_bn_acclimate_nhwc";
  static const char align_rule[] = "x, residual and workspace must be 16-byte aligned, num_batches_dev 8-byte aligned";
  // exactly one pixel: fewer is bn_run's shape refusal
  if (n_pix == 1) { set_error("%s: more than one value per channel is needed to fold an unbiased variance in", who); return DIB_EINVAL; }
  if (bump && !num_batches_dev) { set_error("%s: bump without num_batches_dev", who); return DIB_EINVAL; }
  if (!(momentum <= 1.f)) { set_error("%s: momentum above 1 (negative: cumulative average)", who); return DIB_EINVAL; }
  if (((uintptr_t)num_batches_dev & 7) != 0) { set_error("%s: %s", who, align_rule); return DIB_EINVAL; }
  return bn_run(who, align_rule, x_dev, residual_dev, n_pix, C, running_mean_dev, running_var_dev, relu, bump ? num_batches_dev : nullptr,
                workspace_dev, workspace_bytes, stream, [&](dim3 grid, dim3 block, hipStream_t s, const BnGeom &g, const BnWorkspace &w) {
                  hipLaunchKernelGGL(bn_acclimate_finalize_kernel, grid, block, 0, s, g, w.ws_mean, w.ws_m2, weight_dev, bias_dev,
                                     running_mean_dev, running_var_dev, (const long long *)num_batches_dev, bump ? 1 : 0, momentum, eps,
                                     w.scale, w.shift, stats_dev);
                });
}
