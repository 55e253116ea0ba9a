"""Restoration quality (this repo; `train_deblurrer.py --validate_images`): how close an image is to the sharp one it was made from, as
mean squared error, PSNR and SSIM.  Where the blur runs on the device the sharp image is there right before the blur replaces it, so what
the blur took away and what a deblurrer or Richardson-Lucy (models/deblur.py, models/deconvolve.py) give back are measurable without
leaving the device.  `psnr_ssim` compares one pair and returns its three figures as a device tensor: nothing waits for the device.

The definition (include/dib.h, dib_image_quality; csrc/dib_quality.hip).  A stated reading -- DeepDeblur reports PSNR and SSIM, its loss/
package is not in the reference tree: Wang et al. 2004 as skimage.metrics.structural_similarity(gaussian_weights=True, sigma=1.5,
use_sample_covariance=False, data_range=L, channel_axis=0) computes it.  a, b: planar C x H x W, Half or fp32 each.
    mse = mean (a - b)^2;   psnr_db = 10 log10(L^2 / mse), +inf when mse == 0
    g: 11 taps, g_k ~ exp(-(k - 5)^2 / (2 1.5^2)), sum 1, separable;  every moment mu_a, mu_b, E[aa], E[bb], E[ab] is the VALID 11 x 11
    correlation with g (x) g: (H - 10) x (W - 10) windows per channel
    var_a = E[aa] - mu_a^2, var_b = E[bb] - mu_b^2, cov = E[ab] - mu_a mu_b;  C1 = (0.01 L)^2, C2 = (0.03 L)^2
    S = (2 mu_a mu_b + C1)(2 cov + C2) / ((mu_a^2 + mu_b^2 + C1)(var_a + var_b + C2));   ssim = mean of S over windows and channels
The kernel's arithmetic: pixels as fp32 minus a pivot that all pixels of a window share (today the mean of the 42 x 42 pixel tile a
workgroup stages: an implementation choice, not part of the contract; added back to the means), moments and S in fp32, the two means over the image in fp64; the window's fp32 weights are multiples of 2^-24 that sum to exactly 1
(WINDOW).

CUDA tensors take the HIP entry on the current stream (two launches, no synchronisation, workspace from torch's allocator: capturable);
CPU tensors take `psnr_ssim_torch`, the plain-torch restatement of the definition with the same window, in float64 (in float32 on
request: that form, shifted by L / 2, is what the HIP path's time is measured against on the GPU).

No accuracy claim: PSNR and SSIM of synthetic images say how well a stage restores those images, nothing about detection AP."""
import math

import torch

TAPS = 11
HALO = TAPS - 1
# round(2^24 g_k) with the centre tap taking the residual: the eleven sum to 2^24 (csrc/dib_quality.hip holds the same integers)
_WINDOW_2_24 = (17253, 127486, 603993, 1834768, 3573640, 4462936, 3573640, 1834768, 603993, 127486, 17253)
assert sum(_WINDOW_2_24) == 1 << 24
WINDOW = tuple(v / float(1 << 24) for v in _WINDOW_2_24)


def _check(a, b, data_range):
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float16, torch.float32):
            raise TypeError("psnr_ssim: %s must be a float16 or float32 tensor" % name)
        if t.dim() != 3:
            raise ValueError("psnr_ssim: %s must be planar C x H x W, got %s" % (name, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("psnr_ssim: %s must be contiguous" % name)
    if a.shape != b.shape:
        raise ValueError("psnr_ssim: shapes differ: %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if a.device != b.device:
        raise ValueError("psnr_ssim: the images are on different devices: %s and %s" % (a.device, b.device))
    if a.shape[0] < 1 or a.shape[1] < TAPS or a.shape[2] < TAPS:
        raise ValueError("psnr_ssim: image %s is smaller than the 11 x 11 window" % (tuple(a.shape),))
    L = float(data_range)
    if not (L > 0 and math.isfinite(L)):
        raise ValueError("psnr_ssim: data_range must be positive and finite, got %r" % (data_range,))
    return L


def _valid_correlation(q, dim):
    """sum_k g_k q[.., k : k + n] along `dim`, taps in order, in q's dtype"""
    n = q.shape[dim] - HALO
    acc = q.narrow(dim, 0, n) * WINDOW[0]
    for k in range(1, TAPS):
        acc = torch.add(acc, q.narrow(dim, k, n), alpha=WINDOW[k])
    return acc


@torch.no_grad()
def psnr_ssim_torch(a, b, data_range=1.0, out=None, dtype=torch.float64):
    """The definition in plain torch ops on the images' device (CPU or GPU): pixels minus L / 2 (added back to the means), moments and S
    in `dtype`, the two means over the image in float64.  No host synchronisation."""
    L = _check(a, b, data_range)
    half = 0.5 * L
    a32, b32 = a.to(dtype), b.to(dtype)
    d = a32 - b32
    mse = (d * d).double().mean()
    x, y = a32 - half, b32 - half
    m = _valid_correlation(_valid_correlation(torch.stack([x, y, x * x, y * y, x * y]), 3), 2)
    var_a, var_b, cov = m[2] - m[0] * m[0], m[3] - m[1] * m[1], m[4] - m[0] * m[1]
    mu_a, mu_b = m[0] + half, m[1] + half
    c1, c2 = _constants(L)
    S = ((2.0 * (mu_a * mu_b) + c1) * (2.0 * cov + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2))
    ssim = S.double().mean()
    psnr = 10.0 * torch.log10(L * L / mse)           # mse == 0: +inf; NaN: NaN
    res = torch.stack([mse, psnr, ssim]).float()
    if out is None:
        return res
    _check_out(out, a)
    out.copy_(res)
    return out


def _constants(L):
    """C1, C2 as the kernel forms them: fp32 products"""
    f = torch.tensor([0.01, 0.03], dtype=torch.float32) * torch.tensor(L, dtype=torch.float32)
    f = f * f
    return float(f[0]), float(f[1])


def _check_out(out, a):
    if out.dtype != torch.float32 or out.numel() != 3 or not out.is_contiguous() or out.device != a.device:
        raise ValueError("psnr_ssim: out must be 3 contiguous float32 elements on the images' device")


def workspace_bytes(C, H, W):
    from . import _lib
    return int(_lib.lib().dib_image_quality_workspace_bytes(int(C), int(H), int(W)))


@torch.no_grad()
def psnr_ssim_hip(a, b, data_range=1.0, out=None, work=None):
    """dib_image_quality on two CUDA images, on the current stream.  `work`: a CUDA byte tensor of at least workspace_bytes(C, H, W)
    bytes, 8-byte aligned (None: from torch's allocator)."""
    from . import _lib, blur_ops
    L = _check(a, b, data_range)
    if not a.is_cuda:
        raise TypeError("psnr_ssim_hip needs CUDA images")
    C, H, W = (int(v) for v in a.shape)
    if out is None:
        out = torch.empty(3, dtype=torch.float32, device=a.device)
    else:
        _check_out(out, a)
    need = workspace_bytes(C, H, W)
    if work is None:
        work = torch.empty(need // 8, dtype=torch.float64, device=a.device)
    elif work.numel() * work.element_size() < need or not work.is_contiguous() or work.device != a.device:
        raise ValueError("psnr_ssim_hip: work must hold %d contiguous bytes on the images' device" % need)
    _lib.check(_lib.lib().dib_image_quality(a.data_ptr(), blur_ops._DT[a.dtype], b.data_ptr(), blur_ops._DT[b.dtype], C, H, W, L,
                                            out.data_ptr(), work.data_ptr(), _lib.stream_of(a)))
    return out


def psnr_ssim(a, b, data_range=1.0, out=None):
    """a, b: planar C x H x W, contiguous, Half or fp32 each, on one device.  Returns (or fills `out` with) 3 fp32 elements on that
    device: mse, psnr_db, ssim.  CUDA images take the HIP entry (an error when the library is missing: there is no fallback); CPU images
    the torch restatement.  ValueError: H or W < 11, shapes that differ, input that is not planar or not contiguous."""
    if isinstance(a, torch.Tensor) and a.is_cuda:
        return psnr_ssim_hip(a, b, data_range, out)
    return psnr_ssim_torch(a, b, data_range, out)
