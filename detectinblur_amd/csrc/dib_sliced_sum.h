// The deterministic "sliced sum" of the DeepDeblur trainer's kernels -- the bias gradient and the L1 loss (dib_deblur_train.hip), the
// adversarial loss (dib_deblur_adv.hip) -- stated once.  No float atomics.
//
// THE SUMMATION ORDER is fixed by the shape alone, so two calls on the same input agree bit for bit.  n items in memory order are cut
// into S slices of consecutive items, the first n % S one item longer (slice_begin).  A workgroup of 256 lanes takes one slice as R rows
// of lanes: row r adds the items slice_begin + r, + R, + 2 R, ... one after the other, a chain of at most L = ceil(slice length / R)
// additions.  The R rows are then added in LDS as a tree (row_tree: row r takes row r + h for h = the powers of two below R, largest
// first, only where r + h < R): ceil(log2 R) levels.  A second launch adds the S slice sums in slice order from slice 0: S - 1 additions.
//     DEPTH of the tree, the number of fp32 additions any one input can pass through:  L + ceil(log2 R) + S - 1.
//     Every addition rounds once, so |sum - exact| <= depth * 2^-24 * sum |item| (first order in 2^-24).
//   bias gradient   an item is a pixel of the [n_pix][C] gradient, and each of a workgroup's QB = min(C / V, 256) lane columns sums V
//                   channels of its own: R = 256 / QB, S = slice_count(n_pix, 16 R).  V = 4 when C % 4 == 0, else 1; the Half form,
//                   dib_bias_grad_f16_nhwc: V = 8 when C % 8 == 0 and the gradient is 16-byte aligned, else 1 -- one 16-byte load per
//                   lane either way, and every Half is exact in fp32, so only the additions round.  The slice sums go to the
//                   workspace [S][C]; bias_grad_final_kernel adds them for each channel.
//   scalar losses   (dib_l1_pyramid_loss: n = 3 n_pix differences; dib_adv_bce_loss: n logits)  an item is one element's term; R = 256,
//                   a tree of 8 levels; S = slice_count(n, 2048).  sliced_sum_final_kernel adds the S sums, divides by float(n) and
//                   adds the result onto the loss scalar: L + 8 + S - 1 additions, then one division and one addition.
// models/deblur_train.py restates the geometries (bias_grad_depth, sliced_sum_depth) for the tests' error bounds.  The order itself is
// restated in numpy float32 from this comment (tests/test_deblur_train.py: _walk); tests/test_deblur_train_geometry_gpu.py and
// tests/test_deblur_adversarial_gpu.py hold the kernels to it bit for bit up to S = 1024: change the order here and there together.
#pragma once
#include "dib_common.h"

namespace dib {

constexpr int SS_THREADS = 256, SS_MAX_SLICES = 1024, SS_ELEMS_PER_LANE = 8;

// (static: dib_bnstats.hip keeps a slice_begin of its own in this namespace, with another rule and pins of its own)
static __host__ __device__ inline long long slice_begin(long long n, int S, int s) { return n / S * s + (n % S < s ? n % S : s); }

inline int slice_count(long long n, long long per_slice) {
  long long S = (n + per_slice - 1) / per_slice;
  if (S > SS_MAX_SLICES) S = SS_MAX_SLICES;
  return S < 1 ? 1 : (int)S;
}
inline int scalar_slices(long long n) { return slice_count(n, (long long)SS_THREADS * SS_ELEMS_PER_LANE); }      // the workspace's floats

struct ScalarSum { static __device__ __forceinline__ float add(float a, float b) { return a + b; } };

// The tree over the R rows of `sh`, one value per lane; lane t sits in row `row`, and the same column of the next row is QB lanes on.
// One barrier per level; the caller has stored sh[t] and passed a barrier.  The result is in row 0.
template <class Ops, typename T>
__device__ __forceinline__ void row_tree(T *sh, int t, int row, bool active, int R, int QB) {
  int h = 1;
  while (h < R) h <<= 1;
  for (h >>= 1; h >= 1; h >>= 1) {
    if (active && row < h && row + h < R) sh[t] = Ops::add(sh[t], sh[t + h * QB]);
    __syncthreads();
  }
}

// The scalar losses.  `term(e)` loads element e, stores its gradient element and returns its addend.
template <class Term>
__global__ __launch_bounds__(SS_THREADS) void sliced_sum_partial_kernel(const Term term, long long n, int S, float *__restrict__ partial) {
  __shared__ float sh[SS_THREADS];
  const int t = threadIdx.x, s = blockIdx.x;
  const long long e1 = slice_begin(n, S, s + 1);
  float acc = 0.f;
  for (long long e = slice_begin(n, S, s) + t; e < e1; e += SS_THREADS) acc += term(e);
  sh[t] = acc;
  __syncthreads();
  row_tree<ScalarSum>(sh, t, t, true, SS_THREADS, 1);      // R = 256: r + h < R holds at every level
  if (t == 0) partial[s] = sh[0];
}

// `Term` only names the loss in a profile.
template <class Term>
__global__ void sliced_sum_final_kernel(const float *__restrict__ partial, int S, float n, float *loss) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float acc = partial[0];
  for (int s = 1; s < S; ++s) acc += partial[s];
  *loss = *loss + acc / n;
}

// Both launches; `work`: scalar_slices(n) floats.  The caller has checked the pointers.
template <class Term>
static int sliced_sum_run(const Term &term, long long n, float *loss, float *work, hipStream_t stream) {
  const int S = scalar_slices(n);
  hipLaunchKernelGGL(sliced_sum_partial_kernel<Term>, dim3((unsigned)S), dim3(SS_THREADS), 0, stream, term, n, S, work);
  DIB_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(sliced_sum_final_kernel<Term>, dim3(1), dim3(64), 0, stream, (const float *)work, S, (float)n, loss);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}

}  // namespace dib
