// DeepDeblur's adversarial loss (`train_deblurrer.py --loss ...+w*ADV`, models/deblur_adversarial.py): what the discriminator's step
// runs around MIOpen's convolutions.  HBM-bound streams; no scratch, no float atomics, no host synchronisation, everything on the
// caller's stream (capturable).
//
//   (a) leaky_fwd_kernel     LeakyReLU in place on a convolution output, x = x > 0 ? x : x * slope, one 16-byte vector per lane (4 fp32
//                            or 8 Half; Half is upcast, multiplied in fp32 and rounded once), and on request the sign pattern of the
//                            STORED values beside it, one byte per vector (the layout of dib_bias_act_mask_nhwc): what the backward
//                            needs of the activation, at 1/16 of its size.  NaN stays NaN.  -0 stays -0 in fp32; the Half
//                            form gives +0, because torch's own Half kernel on this GPU does (`leak` below), and the plain module
//                            is what this path is held to bit for bit.
//   (b) leaky_bwd_kernel     its backward from that mask: out = bit ? g : g * slope.  out may be g.  For slope > 0 the sign of the
//                            result is the sign of the input, so the mask of the result serves (slope <= 0 is refused).
//   (c) sliced_sum_partial_kernel<BceTerm> + sliced_sum_final_kernel
//                            binary cross-entropy with logits against a CONSTANT label (1: "real", 0: "fake"), mean over n, added into
//                            a device scalar, with the gradient stored beside it.  With z = -x for label 1 and z = x for label 0:
//                                term    = softplus(z) = max(z, 0) + log1p(exp(-|z|))
//                                grad[i] = (label 1: -1, label 0: +1) * k * sigma(z),   k = gscale / float(n) (one fp32 division),
//                                sigma(z) = z >= 0 ? 1 / (1 + e) : e / (1 + e),  e = exp(-|z|)      (no overflow: e <= 1)
//                            A NaN logit gives a NaN at its own gradient element and a NaN loss, nothing else.  +-inf follows the
//                            formulas: z = +inf gives term inf and sigma 1, z = -inf gives term 0 and sigma 0 (torch's
//                            binary_cross_entropy_with_logits gives NaN there: not compared).
//
// THE SUMMATION ORDER of (c), fixed by n alone, is the scalar losses' of dib_sliced_sum.h -- dib_l1_pyramid_loss's, by the same kernels;
// models/deblur_adversarial.py restates its depth as `adv_loss_depth`.
#include "dib_eltwise_vec.h"      // F32Lane, F16Lane (unpack, pack, sign_mask); args_ok, grid_1d, launch
#include "dib_sliced_sum.h"
#include <cmath>
#include <type_traits>

namespace dib {

// ---- (a), (b) LeakyReLU with a sign mask -----------------------------------------------------------------------------------------
// The product of the negative branch.  fp32: x * slope.  Half: torch's LeakyReLU kernels, forward and backward, return +0 for a Half -0
// on gfx950 where IEEE's product is -0, and equal x * slope, rounded once, at each of the other 65535 Half values
// (tests/test_deblur_adversarial_gpu.py compares them all): the arithmetic of a multiply-add onto +0, which is restated here.
// -ffp-contract=off keeps the sum apart from the product; x + 0 == x for every x but -0.
template <class L>
__device__ __forceinline__ float leak(float v, float slope) {
  return std::is_same<L, F16Lane>::value ? v * slope + 0.f : v * slope;
}

template <class L, bool MASK>
__global__ __launch_bounds__(256) void leaky_fwd_kernel(typename L::Raw *__restrict__ x, long long n, float slope,
                                                       unsigned char *__restrict__ mask) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    float v[L::N];
    L::unpack(x[i], v);
#pragma unroll
    for (int k = 0; k < L::N; ++k) v[k] = v[k] > 0.f ? v[k] : leak<L>(v[k], slope);
    const typename L::Raw o = L::pack(v);
    x[i] = o;
    if (MASK) mask[i] = (unsigned char)L::sign_mask(o);
  }
}

// g and out may be the same tensor (no __restrict__): a lane reads its vector before it writes it, and no other lane touches it.
template <class L>
__global__ __launch_bounds__(256) void leaky_bwd_kernel(const typename L::Raw *g, const unsigned char *__restrict__ mask, float slope,
                                                       typename L::Raw *out, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    float v[L::N];
    L::unpack(g[i], v);
    const unsigned m = mask[i];
#pragma unroll
    for (int k = 0; k < L::N; ++k) v[k] = ((m >> k) & 1u) ? v[k] : leak<L>(v[k], slope);
    out[i] = L::pack(v);
  }
}

static bool leaky_shape_ok(const char *who, float slope, long long n_elems, int lane) {
  if (!std::isfinite(slope) || !(slope > 0.f)) {
    set_error("%s: slope %g: needs a finite slope above 0 (the mask of the result is the mask of the input only then)", who, (double)slope);
    return false;
  }
  if (n_elems < 0 || (n_elems % lane) != 0) { set_error("%s: n_elems must be a non-negative multiple of %d", who, lane); return false; }
  return true;
}

template <class L>
static int leaky_forward(const char *who, void *x, long long n_elems, float slope, unsigned char *mask, void *stream) {
  if (!leaky_shape_ok(who, slope, n_elems, L::N)) return DIB_EINVAL;
  int code;
  if (!args_ok(who, n_elems == 0, {x}, {x}, &code)) return code;
  return launch(mask ? leaky_fwd_kernel<L, true> : leaky_fwd_kernel<L, false>, grid_1d(n_elems / L::N), stream, x, n_elems / L::N, slope, mask);
}

template <class L>
static int leaky_backward(const char *who, const void *g, const unsigned char *mask, float slope, void *out, long long n_elems, void *stream) {
  if (!leaky_shape_ok(who, slope, n_elems, L::N)) return DIB_EINVAL;
  int code;
  if (!args_ok(who, n_elems == 0, {g, mask, out}, {g, out}, &code)) return code;
  return launch(leaky_bwd_kernel<L>, grid_1d(n_elems / L::N), stream, g, mask, slope, out, n_elems / L::N);
}

// ---- (c) binary cross-entropy with logits against a constant label ----------------------------------------------------------------
struct BceTerm {
  const float *logits;
  int real_label;
  float k;
  float *grad;
  __device__ __forceinline__ float operator()(long long i) const {
    const float ks = real_label ? -k : k;
    const float x = logits[i];
    const float z = real_label ? -x : x;
    const float e = expf(-fabsf(z));               // in (0, 1]; NaN for a NaN logit
    const float d = 1.f + e;
    grad[i] = ks * (z >= 0.f ? 1.f / d : e / d);   // a NaN z takes the second branch: NaN / NaN
    return fmaxf(z, 0.f) + log1pf(e);              // fmaxf drops a NaN, log1pf(e) brings it back
  }
};

}  // namespace dib

using namespace dib;

extern "C" int dib_leaky_relu_mask(float *x_dev, long long n_elems, float slope, unsigned char *mask_dev, void *stream) {
  return leaky_forward<F32Lane>("dib_leaky_relu_mask", x_dev, n_elems, slope, mask_dev, stream);
}

extern "C" int dib_leaky_relu_mask_f16(void *x_dev, long long n_elems, float slope, unsigned char *mask_dev, void *stream) {
  return leaky_forward<F16Lane>("dib_leaky_relu_mask_f16", x_dev, n_elems, slope, mask_dev, stream);
}

extern "C" int dib_leaky_relu_mask_backward(const float *grad_dev, const unsigned char *mask_dev, float slope, float *out_dev, long long n_elems,
                                            void *stream) {
  return leaky_backward<F32Lane>("dib_leaky_relu_mask_backward", grad_dev, mask_dev, slope, out_dev, n_elems, stream);
}

extern "C" int dib_leaky_relu_mask_backward_f16(const void *grad_dev, const unsigned char *mask_dev, float slope, void *out_dev, long long n_elems,
                                                void *stream) {
  return leaky_backward<F16Lane>("dib_leaky_relu_mask_backward_f16", grad_dev, mask_dev, slope, out_dev, n_elems, stream);
}

extern "C" size_t dib_adv_bce_loss_workspace_bytes(long long n) {
  if (n <= 0) return 0;
  return (size_t)scalar_slices(n) * sizeof(float);
}

extern "C" int dib_adv_bce_loss(const float *logits_dev, long long n, int real_label, float gscale, float *grad_dev, float *loss_dev,
                                void *work_dev, void *stream) {
  static const char who[] = "dib_adv_bce_loss";
  if (n <= 0 || n > (1ll << 40)) { set_error("%s: needs 0 < n <= 2^40", who); return DIB_EINVAL; }
  if (real_label != 0 && real_label != 1) { set_error("%s: real_label %d (1: real, 0: fake)", who, real_label); return DIB_EINVAL; }
  if (!logits_dev || !grad_dev || !loss_dev || !work_dev) { set_error("%s: null pointer", who); return DIB_EINVAL; }
  const uintptr_t bits = (uintptr_t)logits_dev | (uintptr_t)grad_dev | (uintptr_t)loss_dev | (uintptr_t)work_dev;
  if ((bits & 3) != 0) { set_error("%s: tensors must be 4-byte aligned", who); return DIB_EINVAL; }
  return sliced_sum_run(BceTerm{logits_dev, real_label, gscale / (float)n, grad_dev}, n, loss_dev, (float *)work_dev, (hipStream_t)stream);
}
