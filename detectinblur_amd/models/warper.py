""""Squint" warper (`--warp_in_model`): stretches the image along the blur's principal axes before
the backbone and un-stretches every feature map after it -- SURVEY.md section 8f-2, reference
models/warper.py:13-52 and models/generalized_rcnn.py:131-141.  It consumes the
`theta_rad / scale_factor_lambda1 / scale_factor_lambda2` that `transforms.BlurImage` already
computes for the hot path.

The transform, per image, in homogeneous 3 x 3 form (all matrices Half, as the reference keeps them):
    S = diag(l1, l2, 1)                                   anisotropic scale
    R = rotation by -theta
    T = identity with (width, height) in the LAST ROW     (the reference's placement, kept as is)
    F = R @ T,  G = S @ F,  M = inv(inv(F) @ G)           both inverses in float32, results cast to Half
and the top two rows of M drive `affine_grid` + bilinear `grid_sample` (zeros outside, align_corners
False), computed in Half and returned as float32.

Two paths.  `Warper()` is the stock PyTorch op chain above.  `Warper(fused=True)` (what the detector
builds) sends a float32 GPU tensor through ONE HIP launch instead (csrc/dib_warp.hip; DESIGN.md
section 4): the Half grid coordinates of the chain are reproduced exactly (`squint_half_grid` is
that arithmetic as a torch function), the sampling runs in float32, and nothing but the input is
read and the output written.
"""
import os

import torch
from torch import nn
import torch.nn.functional as F


def squint_matrices(thetas, lambda1s, lambda2s, width, height):
    """[B, 2, 3] Half affine matrices of the warp described in the module docstring."""
    B = lambda1s.shape[0]
    dt, dev = lambda1s.dtype, lambda1s.device

    def eye():
        m = torch.zeros((B, 3, 3), dtype=dt, device=dev)
        m[:, 0, 0] = 1; m[:, 1, 1] = 1; m[:, 2, 2] = 1
        return m

    scale = eye()
    scale[:, 0, 0] = lambda1s
    scale[:, 1, 1] = lambda2s
    t = -thetas
    c, s = torch.cos(t), torch.sin(t)
    rot = eye()
    rot[:, 0, 0] = c; rot[:, 0, 1] = -s
    rot[:, 1, 0] = s; rot[:, 1, 1] = c
    trans = eye()
    trans[:, 2, 0] = torch.ones_like(lambda1s) * width
    trans[:, 2, 1] = torch.ones_like(lambda1s) * height
    fwd = torch.bmm(rot, trans)
    fwd_scaled = torch.bmm(scale, fwd)
    overall = torch.bmm(torch.inverse(fwd.float()).to(dt), fwd_scaled)
    overall = torch.inverse(overall.float()).to(dt)
    return overall[:, 0:2, :]


_BASE_GRIDS = {}     # (H, W, device) -> (bx [W], by [H]) Half tables; a handful of geometries per run (the image and five levels)


def _base_axis(n):
    # torch's linspace_from_neg_one (aten/src/ATen/native/AffineGridGenerator.cpp) for align_corners False, in Half
    if n <= 1:
        return torch.zeros(1, dtype=torch.float16)
    return torch.linspace(-1, 1, n, dtype=torch.float16) * (n - 1) / n


def squint_base_grid(H, W, device="cpu"):
    """The Half base coordinates `affine_grid` gives the columns (bx [W]) and rows (by [H]) of an H x W output.  Built on the
    CPU with torch's own expression -- so they are the reference's on every device; the closed form half((2 j + 1) / W - 1)
    differs from it in 614 of 1344 entries -- and uploaded once per geometry and device."""
    key = (int(H), int(W), torch.device(device))
    tables = _BASE_GRIDS.get(key)
    if tables is None:
        tables = _BASE_GRIDS[key] = (_base_axis(int(W)).to(key[2]), _base_axis(int(H)).to(key[2]))
    return tables


def squint_half_grid(m, H, W):
    """[B, H, W, 2] Half sampling grid of the Half matrices m [B, 2, 3]: what `F.affine_grid(m, (B, C, H, W),
    align_corners=False).float().half()` returns on the CPU, bit for bit (tests/test_squint_warp.py), written out as the
    arithmetic the HIP kernel does per pixel: float32 sums of the (exact) float32 products of two Halves, left to right, one
    rounding to Half.  The executable statement of the kernel's coordinates; used by tests, not on the hot path."""
    bx, by = squint_base_grid(H, W, m.device)
    bx, by, mf = bx.float()[None, None, :], by.float()[None, :, None], m.float()[:, :, :, None, None]
    gx = (mf[:, 0, 0] * bx + mf[:, 0, 1] * by) + mf[:, 0, 2]
    gy = (mf[:, 1, 0] * bx + mf[:, 1, 1] * by) + mf[:, 1, 2]
    return torch.stack((gx, gy), dim=-1).half()


def _layout_of(x):
    """The kernels' layout code of a float32 GPU tensor they take as it lies in memory, else None."""
    from .. import _lib
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.numel() > 0):
        return None
    if x.is_contiguous():           # also what a one-channel or 1 x 1 channels-last tensor is
        return _lib.DIB_WARP_NCHW
    if x.is_contiguous(memory_format=torch.channels_last):
        return _lib.DIB_WARP_NHWC
    return None


def squint_warp_launch(x, m):
    """One forward launch: x float32 [N, C, H, W] (contiguous or channels-last) warped by the Half matrices m [N, 2, 3], which
    the kernel reads from device memory when it RUNS -- a captured graph follows the contents of `m`.  Returns (out, tables)."""
    from .. import _lib
    N, C, H, W = x.shape
    layout = _layout_of(x)
    if layout is None:
        raise ValueError("squint_warp_launch: needs a dense float32 GPU tensor (contiguous or channels-last), got %s %s strides %s"
                         % (x.device, x.dtype, tuple(x.stride())))
    assert m.dtype == torch.float16 and m.is_contiguous() and tuple(m.shape) == (N, 2, 3) and m.device == x.device
    tables = squint_base_grid(H, W, x.device)
    out = torch.empty_like(x)          # preserve_format: the input's layout
    _lib.check(_lib.lib().dib_squint_warp_forward(x.data_ptr(), out.data_ptr(), N, C, H, W, layout, m.data_ptr(), tables[0].data_ptr(),
                                                  tables[1].data_ptr(), _lib.stream_of(x)))
    return out, tables


class _SquintWarp(torch.autograd.Function):
    """include/dib.h: dib_squint_warp_forward / _backward.  The float32 result is returned as the kernel sums it: the reference
    rounds it to Half once more (a relative 2^-11, below the CPU-versus-GPU difference of torch's own Half kernels that
    tests/test_warper.py accepts).  Backward: float atomic adds into a zero-filled gradient, launched only if x needs one."""

    @staticmethod
    def forward(ctx, x, m):
        out, tables = squint_warp_launch(x, m)
        ctx.save_for_backward(m, *tables)
        ctx.layout = _layout_of(x)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from .. import _lib
        m, bx, by = ctx.saved_tensors
        fmt = torch.channels_last if ctx.layout == _lib.DIB_WARP_NHWC else torch.contiguous_format
        g = grad_out.float().contiguous(memory_format=fmt)
        N, C, H, W = g.shape
        grad = torch.zeros_like(g)
        _lib.check(_lib.lib().dib_squint_warp_backward(g.data_ptr(), grad.data_ptr(), N, C, H, W, ctx.layout, m.data_ptr(), bx.data_ptr(),
                                                       by.data_ptr(), _lib.stream_of(g)))
        return grad, None


class Warper(nn.Module):
    def __init__(self, fused=False):
        super().__init__()
        self.fused = fused

    def takes_fused(self, x):
        """Whether this call goes through the HIP kernels: a fused warper, a float32 GPU tensor in a layout they read as it
        lies, and no DIB_NO_FUSED_WARP=1 in the environment.  (The library failing to load is an error, not a reason.)"""
        return self.fused and _layout_of(x) is not None and os.environ.get("DIB_NO_FUSED_WARP") != "1"

    def forward(self, x, thetas, lambda1s, lambda2s):
        height, width = x.shape[-2], x.shape[-1]
        m = squint_matrices(thetas, lambda1s, lambda2s, width, height)
        if self.takes_fused(x):
            return _SquintWarp.apply(x, m.to(device=x.device, dtype=torch.float16).contiguous())
        grid = F.affine_grid(theta=m, size=x.shape, align_corners=False).float().half()
        out = F.grid_sample(x.half(), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        return out.float()
