// Detection overlays (reference engine.py:382-383 around utils.py:322-353): the picture `evaluate` saves of every image it scores -- the
// planar fp16 / fp32 image as the detector saw it, turned into tight interleaved 8-bit RGB with the box outlines already in it, ONE
// launch for up to MAX_BATCH images.  Pixel value and outline rule: include/dib.h.
//
// A memory-bound stream (6 or 12 bytes in, 3 bytes out per pixel).  An image is walked as a FLAT run of H * W pixels, 1,024 per
// workgroup, four consecutive pixels per lane: the lane's 12 output bytes are three aligned dwords wherever the rows fall, and its four
// elements per plane are one 8- / 16-byte load where H * W % 4 == 0 and the plane is aligned (the element path otherwise; the last
// H * W % 4 pixels of an image are stored byte by byte).
// Boxes: a pixel never tests every box.  A workgroup covers a span of rows; it culls the image's boxes against that span into LDS, in
// chunks of 256 from the LAST chunk to the first, keeping drawing order inside a chunk (wave ballots); its lanes walk the survivors from
// last to first and stop at the first one that paints each of their pixels -- the last painting box in drawing order, as a sequence of
// cv2.rectangle calls leaves it.  Most workgroups of an evaluation picture keep no box at all and skip the loop.
#include <hip/hip_fp16.h>

#include "dib_common.h"

namespace dib {

constexpr int OVL_LANES = 256, OVL_PIX = 4, OVL_BLOCK_PIX = OVL_LANES * OVL_PIX, OVL_COORD_MAX = 1 << 30;

struct OverlayImage {
  const void *in;
  unsigned char *out;
  int H, W;
  int box_begin, box_end;
  int vec;             // bit 0: planes take 4-element vector loads; bit 1: out takes dword stores
};

struct OverlayBatch {
  OverlayImage img[MAX_BATCH];
  int block_begin[MAX_BATCH + 1];   // first workgroup of image i (+ total)
  int n;
};

// k = trunc(float(x) * 255), saturated to 0..255, NaN -> 0 (both comparisons are false for a NaN)
__device__ __forceinline__ unsigned to_u8(float x) {
  const float v = x * 255.0f;
  return v >= 255.0f ? 255u : (v > 0.0f ? (unsigned)(int)v : 0u);
}

template <typename T> __device__ __forceinline__ float elem_to_float(T v);
template <> __device__ __forceinline__ float elem_to_float<__half>(__half v) { return __half2float(v); }
template <> __device__ __forceinline__ float elem_to_float<float>(float v) { return v; }

// four consecutive elements of one plane, as floats
__device__ __forceinline__ void load4(const __half *p, float v[4]) {
  const uint2 w = *reinterpret_cast<const uint2 *>(p);
  v[0] = __half2float(__ushort_as_half((unsigned short)(w.x & 0xffffu)));
  v[1] = __half2float(__ushort_as_half((unsigned short)(w.x >> 16)));
  v[2] = __half2float(__ushort_as_half((unsigned short)(w.y & 0xffffu)));
  v[3] = __half2float(__ushort_as_half((unsigned short)(w.y >> 16)));
}
__device__ __forceinline__ void load4(const float *p, float v[4]) {
  const float4 w = *reinterpret_cast<const float4 *>(p);
  v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
}

// does the outline of box b = (xa, ya, xb, yb) paint pixel (x, y)?  include/dib.h states the rule
__device__ __forceinline__ bool outline_paints(const int4 b, int x, int y) {
  const bool outer = x >= b.x - 1 && x <= b.z + 1 && y >= b.y - 1 && y <= b.w + 1;
  const bool inner = x >= b.x + 2 && x <= b.z - 2 && y >= b.y + 2 && y <= b.w - 2;
  const bool corner = (x == b.x - 1 || x == b.z + 1) && (y == b.y - 1 || y == b.w + 1);
  return outer && !inner && !corner;
}

template <typename T>
__global__ __launch_bounds__(OVL_LANES) void overlay_rgb8_kernel(const OverlayBatch batch, const dib_overlay_box *__restrict__ boxes) {
  __shared__ int4 s_box[OVL_LANES];
  __shared__ unsigned s_rgb[OVL_LANES];
  __shared__ int s_wave[OVL_LANES / 64];

  const int blk = blockIdx.x, tid = threadIdx.x;
  int i = 0;
  while (i + 1 < batch.n && blk >= batch.block_begin[i + 1]) ++i;      // workgroup-uniform
  const OverlayImage im = batch.img[i];
  const int W = im.W, npix = im.H * W;                                 // H * W <= 2^30 (checked by the host)
  const int first = (blk - batch.block_begin[i]) * OVL_BLOCK_PIX;      // < npix: the grid holds no empty workgroup
  const int last = min(first + OVL_BLOCK_PIX, npix) - 1;
  const int row_lo = first / W, row_hi = last / W;                     // the rows this workgroup touches

  const int p0 = first + tid * OVL_PIX;
  const int count = min(max(npix - p0, 0), OVL_PIX);                   // pixels of this lane (0: nothing to do but the barriers)
  int px[OVL_PIX], py[OVL_PIX];
  {
    int y = p0 / W, x = p0 - y * W;
#pragma unroll
    for (int k = 0; k < OVL_PIX; ++k) {
      px[k] = x; py[k] = y;
      if (++x == W) { x = 0; ++y; }
    }
  }

  const bool one_row = py[0] == py[OVL_PIX - 1];
  const int lx0 = one_row ? px[0] : 0, lx1 = one_row ? px[OVL_PIX - 1] : W - 1, ly0 = py[0], ly1 = py[OVL_PIX - 1];

  // ---- the pixels: loads issued first, in flight while the boxes are culled ----
  const T *in = static_cast<const T *>(im.in);
  float ch[3][OVL_PIX];
  if (count == OVL_PIX && (im.vec & 1)) {
#pragma unroll
    for (int c = 0; c < 3; ++c) load4(in + (size_t)c * npix + p0, ch[c]);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < OVL_PIX; ++k) ch[c][k] = k < count ? elem_to_float<T>(in[(size_t)c * npix + p0 + k]) : 0.f;
  }

  // ---- boxes: cull a chunk against the workgroup's rows, walk the survivors last to first ----
  unsigned color[OVL_PIX] = {0u, 0u, 0u, 0u};
  unsigned open = (1u << count) - 1u;                                  // bit k: pixel k has no painting box yet; a found pixel is closed
  unsigned painted = 0u;
  const int nbox = im.box_end - im.box_begin;
  for (int base = ((nbox - 1) / OVL_LANES) * OVL_LANES; nbox > 0 && base >= 0; base -= OVL_LANES) {
    const int j = base + tid;
    bool keep = false;
    int4 b = make_int4(0, 0, 0, 0);
    unsigned rgb = 0u;
    if (j < nbox) {
      const dib_overlay_box raw = boxes[im.box_begin + j];
      // corners beyond +-2^30 are taken as +-2^30 (no image reaches that far): the +-2 of the rule cannot overflow
      const int x0 = min(max(raw.x0, -OVL_COORD_MAX), OVL_COORD_MAX), x1 = min(max(raw.x1, -OVL_COORD_MAX), OVL_COORD_MAX);
      const int y0 = min(max(raw.y0, -OVL_COORD_MAX), OVL_COORD_MAX), y1 = min(max(raw.y1, -OVL_COORD_MAX), OVL_COORD_MAX);
      b = make_int4(min(x0, x1), min(y0, y1), max(x0, x1), max(y0, y1));
      rgb = raw.rgb & 0xffffffu;
      keep = b.y - 1 <= row_hi && b.w + 1 >= row_lo && b.x - 1 <= W - 1 && b.z + 1 >= 0;
    }
    // order-preserving compaction: rank inside the wave from the ballot, wave offsets through LDS
    const unsigned long long vote = __ballot(keep);
    const int lane = tid & 63, wave = tid >> 6;
    const int rank = __popcll(vote & ((1ull << lane) - 1ull));
    __syncthreads();                                                   // the previous chunk's survivors have been read by every lane
    if (lane == 0) s_wave[wave] = __popcll(vote);
    __syncthreads();
    int offset = 0, total = 0;
#pragma unroll
    for (int w = 0; w < OVL_LANES / 64; ++w) {
      const int c = s_wave[w];
      if (w < wave) offset += c;
      total += c;
    }
    if (keep) {
      s_box[offset + rank] = b;
      s_rgb[offset + rank] = rgb;
    }
    __syncthreads();
    for (int s = total - 1; s >= 0 && open != 0u; --s) {
      const int4 sb = s_box[s];
      // the lane's four pixels lie in the rectangle [lx0, lx1] x [ly0, ly1]: outside the outline's outer rectangle, or wholly in its
      // interior, none of them is painted -- a wave whose lanes all say so skips the per-pixel test (most waves of a row do)
      if (lx1 < sb.x - 1 || lx0 > sb.z + 1 || ly1 < sb.y - 1 || ly0 > sb.w + 1) continue;
      if (lx0 >= sb.x + 2 && lx1 <= sb.z - 2 && ly0 >= sb.y + 2 && ly1 <= sb.w - 2) continue;
      const unsigned c = s_rgb[s];
#pragma unroll
      for (int k = 0; k < OVL_PIX; ++k) {
        if ((open >> k & 1u) && outline_paints(sb, px[k], py[k])) {
          color[k] = c;
          painted |= 1u << k;
          open &= ~(1u << k);
        }
      }
    }
  }
  if (count == 0) return;

  unsigned v[OVL_PIX];                                                 // R | G << 8 | B << 16: the three output bytes in memory order
#pragma unroll
  for (int k = 0; k < OVL_PIX; ++k) {
    const unsigned own = to_u8(ch[0][k]) | to_u8(ch[1][k]) << 8 | to_u8(ch[2][k]) << 16;
    v[k] = (painted >> k & 1u) ? color[k] : own;
  }
  unsigned char *out = im.out + (size_t)p0 * 3;
  if (count == OVL_PIX && (im.vec & 2)) {
    unsigned *o = reinterpret_cast<unsigned *>(out);                   // p0 % 4 == 0: 12-byte records on a 4-byte aligned base
    o[0] = v[0] | v[1] << 24;
    o[1] = v[1] >> 8 | v[2] << 16;
    o[2] = v[2] >> 16 | v[3] << 8;
  } else {
#pragma unroll
    for (int k = 0; k < OVL_PIX; ++k) {
      if (k < count) {
        out[3 * k + 0] = (unsigned char)(v[k] & 255u);
        out[3 * k + 1] = (unsigned char)(v[k] >> 8 & 255u);
        out[3 * k + 2] = (unsigned char)(v[k] >> 16 & 255u);
      }
    }
  }
}

}  // namespace dib

using namespace dib;

extern "C" int dib_overlay_rgb8(const void *const *in_dev, int dtype, const int *H, const int *W, int B, const dib_overlay_box *boxes_dev,
                                const int *box_offset, unsigned char *const *out_dev, void *stream) {
  const char *who = "dib_overlay_rgb8";
  if (!in_dev || !H || !W || !box_offset || !out_dev) { set_error("%s: null pointer", who); return DIB_EINVAL; }
  if (dtype != DIB_F16 && dtype != DIB_F32) { set_error("%s: unsupported dtype %d", who, dtype); return DIB_EINVAL; }
  if (B < 0 || B > MAX_BATCH) { set_error("%s: B = %d outside 0..%d (split larger lists)", who, B, MAX_BATCH); return DIB_EINVAL; }
  if (B == 0) return DIB_OK;
  if (box_offset[0] < 0) { set_error("%s: box_offset[0] = %d is negative", who, box_offset[0]); return DIB_EINVAL; }
  const size_t elem = dtype == DIB_F16 ? 2 : 4;
  OverlayBatch batch;
  long long blocks = 0;
  for (int i = 0; i < B; ++i) {
    if (!in_dev[i] || !out_dev[i]) { set_error("%s: null pointer (image %d)", who, i); return DIB_EINVAL; }
    if (H[i] <= 0 || W[i] <= 0) { set_error("%s: needs H, W > 0 (image %d: %d x %d)", who, i, H[i], W[i]); return DIB_EINVAL; }
    const long long npix = (long long)H[i] * W[i];
    if (npix > (long long)OVL_COORD_MAX) { set_error("%s: image %d has %lld pixels, more than 2^30", who, i, npix); return DIB_EINVAL; }
    if (box_offset[i + 1] < box_offset[i]) {
      set_error("%s: box_offset decreases at image %d (%d -> %d)", who, i, box_offset[i], box_offset[i + 1]);
      return DIB_EINVAL;
    }
    if ((uintptr_t)in_dev[i] % elem) { set_error("%s: image %d is not aligned to its element size", who, i); return DIB_EINVAL; }
    OverlayImage &im = batch.img[i];
    im.in = in_dev[i]; im.out = out_dev[i]; im.H = H[i]; im.W = W[i];
    im.box_begin = box_offset[i]; im.box_end = box_offset[i + 1];
    im.vec = ((npix % OVL_PIX) == 0 && ((uintptr_t)in_dev[i] % (OVL_PIX * elem)) == 0 ? 1 : 0) | (((uintptr_t)out_dev[i] % 4) == 0 ? 2 : 0);
    batch.block_begin[i] = (int)blocks;
    blocks += (npix + OVL_BLOCK_PIX - 1) / OVL_BLOCK_PIX;
  }
  if (box_offset[B] > box_offset[0] && !boxes_dev) { set_error("%s: null pointer (boxes_dev with %d boxes)", who, box_offset[B] - box_offset[0]); return DIB_EINVAL; }
  for (int i = B; i <= MAX_BATCH; ++i) batch.block_begin[i] = (int)blocks;
  batch.n = B;
  const hipStream_t s = (hipStream_t)stream;
  if (dtype == DIB_F16)
    hipLaunchKernelGGL(overlay_rgb8_kernel<__half>, dim3((unsigned)blocks), dim3(OVL_LANES), 0, s, batch, boxes_dev);
  else
    hipLaunchKernelGGL(overlay_rgb8_kernel<float>, dim3((unsigned)blocks), dim3(OVL_LANES), 0, s, batch, boxes_dev);
  DIB_HIP_CHECK(hipGetLastError());
  return DIB_OK;
}
