// THE PATCH MAP of the DeepDeblur trainer: which source element an element of an output patch comes from, and what the host asks of an
// image before a kernel may follow the map.  Stated once for dib_deblur_patches (dib_deblur_train.hip: patches_kernel, pure data movement)
// and dib_deblur_patches_augment (dib_deblur_augment.hip: patches_augment_kernel, the same movement with the value steps).
// out[c][y][x] = in[order[c]][py + y1][px + x0]: dataCommon.py's order -- crop, hflip (reverse x), vflip (reverse y), rot90 (a
// transpose), channel order -- read backwards from the output element.
#pragma once
#include "dib_common.h"

namespace dib {

constexpr int PATCH_MAX_BATCH = 64;      // descriptors per launch: 64 of 48 bytes are 3 KB of the 4 KB of kernel arguments
struct PatchDesc {
  const void *in;      // planar [3][H][W]
  int H, W, py, px;
  unsigned flags;      // DIB_PATCH_HFLIP | DIB_PATCH_VFLIP | DIB_PATCH_ROT90 | channel order in bits 4..9
  int pad_;
};

// element offset in the planar source image of element (c, y, x) of the ps x ps output patch
__device__ __forceinline__ size_t patch_source(const PatchDesc &d, int ps, int c, int y, int x) {
  const bool rot = d.flags & DIB_PATCH_ROT90;
  const int y2 = rot ? x : y, x2 = rot ? y : x;
  const int y1 = (d.flags & DIB_PATCH_VFLIP) ? ps - 1 - y2 : y2;
  const int x0 = (d.flags & DIB_PATCH_HFLIP) ? ps - 1 - x2 : x2;
  const int cs = (int)((d.flags >> (4 + 2 * c)) & 3u);
  return ((size_t)cs * d.H + (d.py + y1)) * d.W + (d.px + x0);
}

// Image b of a batch: its pointer (aligned to `elem` bytes), geometry and flags into *d.  DIB_OK, DIB_ESHAPE for a patch that leaves
// the image, DIB_EINVAL otherwise (text set).
inline int patch_desc(const char *who, int b, const void *in, size_t elem, int H, int W, int py, int px, unsigned f, int ps, PatchDesc *d) {
  if (!in || ((uintptr_t)in & (elem - 1)) != 0) { set_error("%s: image %d: null or misaligned pointer", who, b); return DIB_EINVAL; }
  if (H < ps || W < ps || py < 0 || px < 0 || py > H - ps || px > W - ps) {
    set_error("%s: image %d: a %d x %d patch at (%d, %d) leaves the %d x %d image", who, b, ps, ps, py, px, H, W);
    return DIB_ESHAPE;
  }
  if ((f & ~(7u | (63u << 4))) != 0 || ((f >> 4) & 3u) == 3u || ((f >> 6) & 3u) == 3u || ((f >> 8) & 3u) == 3u) {
    set_error("%s: image %d: flags 0x%x (three flip bits, three channel indices 0..2 in bits 4..9)", who, b, f);
    return DIB_EINVAL;
  }
  *d = {in, H, W, py, px, f, 0};
  return DIB_OK;
}

}  // namespace dib
