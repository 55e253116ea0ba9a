"""The training path of DeepDeblur's MSResNet (models/deblur.py holds the network and the inference stage; this file leaves both as
they are).  The reference vendors DeepDeblur's trainer beside the inference wrapper (models/deblur/train.py, dataCommon.py,
model.py); `python -m detectinblur_amd.train_deblurrer` is this project's, fed by the GPU blur.  What is here:

  draws     `draw_patch`: one patch origin and one augmentation per image from Python's `random`, in the order of the reference's
            dataCommon.py -- crop (:32-33) draws randrange for py, then for px; augment (:61-68) draws choice for hflip, for vflip and
            for rot90, then shuffles the channel order.  The patch is cropped first, then hflip (reverse x), vflip (reverse y),
            rot90 (a transpose), then the channel order (:76-81).  The HSV saturation change (:72-87) and dataCommon's add_noise are
            NOT built (the first needs scikit-image's colour conversions; noise is the blur stage's own --add_noise).
  patches   `gather_patches`: the patches of a ragged list of images as one planar [B, 3, ps, ps] tensor: dib_deblur_patches on the
            GPU (one launch, bit-exact data movement), `gather_patches_torch` elsewhere and as the reference of the tests.
  pyramid   `patch_levels`: quantise to 8 bits, Gaussian pyramid, minus 127.5, per patch -- the inference stage's steps 1-3
            (dib_deblur_pyramid / deblur.quantise + deblur.pyramid), written into slab b of batched channels-last level tensors
            [B, 6, ps >> s, ps >> s] (coarsest: [B, 3, ...]); channels 3..5 are never written and never read.  n_scales launches per
            patch: no batched pyramid kernel is part of this project.
  network   `msresnet_train_forward(model, input_levels)`: the outputs per level BEFORE MSResNet's `+ 127.5` (the loss is taken on
            the shifted values: the shift cancels in output - target).  Two ways to the same values, as in models/deblur.py:
              * HIP: CUDA, fp32, channels-last levels, n_feats % 4 == 0 and FUSE_DEBLUR_TRAIN.  The convolutions are F.conv2d without
                bias (MIOpen, plain autograd), each followed in place by dib_bias_act_nhwc, or dib_bias_act_mask_nhwc for the ReLU,
                through `_BiasActTrain`, whose backward is ONE pass (dib_bias_grad_nhwc): the ReLU mask applied to the gradient and
                the bias gradient summed from the same read, in an order fixed by the shape.  PixelShuffle and cat stay torch ops.
              * torch: the plain module, everything else.
            `model.last_path` records which of the two ran ("hip" / "torch").
  loss      `pyramid_l1_loss`: sum over levels of mean |output - target| (DeepDeblur's published L1 loss; its loss/ package is not in
            the reference tree: a stated reading).  On the HIP path one autograd node: dib_l1_pyramid_loss per level adds the level's
            mean into one device scalar and stores the gradient, the backward scales it by the incoming gradient.  The gradient is
            sign(d) / (3 n_pix) with sign(+-0) = 0; a NaN difference gives a NaN gradient there, where torch.sign -- and with it the
            plain path's l1_loss backward -- gives 0: the loss is NaN on both paths, and the driver stops at its next read of it.

Summation orders and the depth of their trees (for error bounds): csrc/dib_deblur_train.hip; restated below as `bias_grad_depth`
and `l1_loss_depth`."""
import collections
import ctypes
import math
import random

import torch
import torch.nn.functional as F

from . import deblur

# False: the plain module on the GPU too, for A/B runs.  On: 292.0 against 300.7 ms per step at the trainer's defaults on an MI355X,
# alternated, spread 0.3 % (profiles/deblur_train.txt).
FUSE_DEBLUR_TRAIN = True

PATCH_HFLIP, PATCH_VFLIP, PATCH_ROT90 = 1, 2, 4          # include/dib.h DIB_PATCH_*
PATCH_MAX_BATCH = 64                                     # images per dib_deblur_patches launch

PatchDraw = collections.namedtuple("PatchDraw", "py px hflip vflip rot90 order")


# ---- draws -----------------------------------------------------------------------------------------------------------------------

def draw_patch(h, w, ps):
    """One image's draws, in dataCommon.py's order (crop :32-33, augment :61-68)."""
    py = random.randrange(0, h - ps + 1)
    px = random.randrange(0, w - ps + 1)
    choices = (False, True)
    hflip = random.choice(choices)
    vflip = random.choice(choices)
    rot90 = random.choice(choices)
    order = list(range(3))
    random.shuffle(order)
    return PatchDraw(py, px, hflip, vflip, rot90, tuple(order))


def flags_word(draw):
    o = draw.order
    return (PATCH_HFLIP if draw.hflip else 0) | (PATCH_VFLIP if draw.vflip else 0) | (PATCH_ROT90 if draw.rot90 else 0) \
        | (o[0] << 4) | (o[1] << 6) | (o[2] << 8)


# ---- patches ---------------------------------------------------------------------------------------------------------------------

def gather_patches_torch(images, draws, ps):
    """planar [3, H_b, W_b] images -> [B, 3, ps, ps], op for op what dataCommon.py does to an H x W x 3 array."""
    out = []
    for img, d in zip(images, draws):
        p = img[:, d.py:d.py + ps, d.px:d.px + ps]
        if d.hflip:
            p = p.flip(2)
        if d.vflip:
            p = p.flip(1)
        if d.rot90:
            p = p.transpose(1, 2)
        out.append(p[list(d.order)])
    return torch.stack(out).contiguous()


def gather_patches_device(images, draws, ps):
    from .. import _lib
    first = images[0]
    if first.dtype not in (torch.float16, torch.float32) or any(im.dtype != first.dtype or im.device != first.device or im.dim() != 3
                                                                  or im.shape[0] != 3 for im in images):
        raise ValueError("gather_patches: planar [3, H, W] Half or fp32 images of one dtype on one device")
    images = [im.contiguous() for im in images]
    out = torch.empty((len(images), 3, ps, ps), dtype=first.dtype, device=first.device)
    dtype = _lib.DIB_F16 if first.dtype == torch.float16 else _lib.DIB_F32
    for b0 in range(0, len(images), PATCH_MAX_BATCH):
        ims, ds = images[b0:b0 + PATCH_MAX_BATCH], draws[b0:b0 + PATCH_MAX_BATCH]
        flags = (ctypes.c_uint * len(ims))(*[flags_word(d) for d in ds])
        _lib.check(_lib.lib().dib_deblur_patches(_lib.ptr_array([im.data_ptr() for im in ims]), dtype,
                                                 _lib.int_array([int(im.shape[1]) for im in ims]), _lib.int_array([int(im.shape[2]) for im in ims]),
                                                 _lib.int_array([d.py for d in ds]), _lib.int_array([d.px for d in ds]), flags, len(ims), ps,
                                                 out[b0].data_ptr(), _lib.stream_of(first)))
    return out


def gather_patches(images, draws, ps):
    if images[0].is_cuda:
        return gather_patches_device(images, draws, ps)
    return gather_patches_torch(images, draws, ps)


# ---- pyramid ---------------------------------------------------------------------------------------------------------------------

def _level_shape(B, ps, s, n_scales):
    return (B, 6 if s < n_scales - 1 else 3, ps >> s, ps >> s)


def patch_levels(patches, n_scales):
    """[B, 3, ps, ps] Half or fp32 in [0, 1] (ps a multiple of 2 ** (n_scales - 1)) -> the levels minus 127.5, finest first, as
    channels-last fp32 [B, 6, ps >> s, ps >> s] tensors (coarsest [B, 3, ...]) of which channels 0..2 are written."""
    B, ps = int(patches.shape[0]), int(patches.shape[-1])
    if ps % (1 << (n_scales - 1)):
        raise ValueError("patch size %d is not a multiple of %d" % (ps, 1 << (n_scales - 1)))
    levels = [torch.empty(_level_shape(B, ps, s, n_scales), dtype=torch.float32, device=patches.device, memory_format=torch.channels_last)
              for s in range(n_scales)]
    # the pyramid kernel wants every slab on 16 bytes: 12 (ps >> s)^2 bytes per patch at the coarsest level
    if patches.is_cuda and 1 <= n_scales <= 4 and all((l[0].numel() * 4) % 16 == 0 for l in levels):
        from .. import _lib
        patches = patches.contiguous()
        fn, stream = _lib.lib().dib_deblur_pyramid, _lib.stream_of(patches)
        dtype = _lib.DIB_F16 if patches.dtype == torch.float16 else _lib.DIB_F32
        for b in range(B):
            _lib.check(fn(patches[b].data_ptr(), dtype, ps, ps, n_scales, _lib.ptr_array([l[b].data_ptr() for l in levels]), stream))
        return levels
    for b in range(B):
        for l, v in zip(levels, deblur.pyramid(deblur.quantise(patches[b]), n_scales)):
            l[b, :3] = v - deblur.RGB_RANGE / 2
    return levels


# ---- the epilogue with its one-pass backward ---------------------------------------------------------------------------------------

def _ceil_div(a, b):
    return -(-a // b)


def bias_grad_depth(n_pix, C):
    """Additions any one input of dib_bias_grad_nhwc's channel sum can pass through (csrc/dib_deblur_train.hip, "THE SUMMATION ORDER")."""
    V = 4 if C % 4 == 0 else 1
    QB = min(C // V, 256)
    R = 256 // QB
    S = max(1, min(1024, _ceil_div(n_pix, 16 * R)))
    L = _ceil_div(_ceil_div(n_pix, S), R)
    return L + (R - 1).bit_length() + S - 1


def l1_loss_depth(n_pix):
    """The same for dib_l1_pyramid_loss's sum of |d|; the division and the addition onto the scalar come on top."""
    n = 3 * n_pix
    S = max(1, min(1024, _ceil_div(n, 2048)))
    return _ceil_div(_ceil_div(n, S), 256) + 8 + S - 1


def sign_mask_torch(y):
    """dib_bias_act_mask_nhwc's mask of a [n_pix, C] (C % 4 == 0) tensor: one byte per 4 consecutive elements, bit k = element > 0."""
    bits = (y.reshape(-1, 4) > 0).to(torch.uint8)
    return bits[:, 0] | (bits[:, 1] << 1) | (bits[:, 2] << 2) | (bits[:, 3] << 3)


def bias_grad_torch(grad, mask=None):
    """dib_bias_grad_nhwc restated: grad [n_pix, C] -> (grad_out, bias_grad)."""
    if mask is not None:
        bits = ((mask.reshape(-1, 1) >> torch.arange(4, device=mask.device, dtype=torch.uint8)) & 1).reshape(grad.shape).bool()
        grad = torch.where(bits, grad, torch.zeros((), dtype=grad.dtype, device=grad.device))
    return grad, grad.sum(0)


def l1_level_torch(out, target, gscale=1.0):
    """dib_l1_pyramid_loss restated: out [n_pix, 3], target [n_pix, >= 3] -> (grad, the level's addend to the loss)."""
    d = out - target[:, :3]
    n = torch.tensor(float(out.numel()), dtype=out.dtype)
    k = (torch.tensor(gscale, dtype=out.dtype) / n).to(out.device)
    grad = torch.where(torch.isnan(d), d, torch.sign(d) * k)
    return grad, d.abs().sum() / n.to(out.device)


def bias_grad_device(grad, mask=None, out=None):
    """dib_bias_grad_nhwc on a channels-last [N, C, H, W] (or a [n_pix, C]) fp32 gradient -> (grad_out, bias_grad); `out` may be
    `grad` itself; without a mask nothing is written and `grad` is returned as it came."""
    from .. import _lib
    C = int(grad.shape[1])
    n_pix = grad.numel() // C
    l = _lib.lib()
    bias_grad = torch.empty(C, dtype=torch.float32, device=grad.device)
    work = torch.empty(max(1, l.dib_bias_grad_workspace_bytes(n_pix, C) // 4), dtype=torch.float32, device=grad.device)
    if mask is not None and out is None:
        out = torch.empty_like(grad)
    _lib.check(l.dib_bias_grad_nhwc(grad.data_ptr(), mask.data_ptr() if mask is not None else None, out.data_ptr() if out is not None else None,
                                    n_pix, C, bias_grad.data_ptr(), work.data_ptr(), _lib.stream_of(grad)))
    return (out if out is not None else grad), bias_grad


class _BiasActTrain(torch.autograd.Function):
    """x = act(x + bias[c] (+ residual)) in place on a channels-last fp32 CUDA convolution output (dib_bias_act_nhwc, or
    dib_bias_act_mask_nhwc with the ReLU); the backward is one launch pair over the gradient (dib_bias_grad_nhwc): masked gradient and
    bias gradient from the same read.  Modelled on the trunk's `_BiasAct` (models/backbone.py), which keeps torch's separate sum."""

    @staticmethod
    def forward(ctx, x, bias, residual, relu):
        from .. import _lib
        C = int(x.shape[1])
        res = residual.data_ptr() if residual is not None else None
        ctx.has_res, ctx.masked = residual is not None, bool(relu)
        l, stream = _lib.lib(), _lib.stream_of(x)
        if relu:
            mask = torch.empty(x.numel() // 4, dtype=torch.uint8, device=x.device)
            _lib.check(l.dib_bias_act_mask_nhwc(x.data_ptr(), bias.data_ptr(), res, x.numel(), C, mask.data_ptr(), stream))
            ctx.save_for_backward(mask)
        else:
            _lib.check(l.dib_bias_act_nhwc(x.data_ptr(), bias.data_ptr(), res, x.numel(), C, 0, stream))
        ctx.mark_dirty(x)
        return x

    @staticmethod
    def backward(ctx, grad):
        if not grad.is_contiguous(memory_format=torch.channels_last):
            grad = grad.contiguous(memory_format=torch.channels_last)      # the mask and the channel index are in NHWC element order
        if grad.data_ptr() & 15:
            grad = grad.clone(memory_format=torch.channels_last)
        # not in place: autograd may hand the same gradient tensor to another node
        grad, gb = bias_grad_device(grad, ctx.saved_tensors[0] if ctx.masked else None)
        return grad, gb, (grad if ctx.has_res else None), None


def _bias_act(y, conv, residual=None, relu=False):
    return _BiasActTrain.apply(y, conv.bias, residual, relu)


# ---- the network -----------------------------------------------------------------------------------------------------------------

def _hip_ok(model, levels):
    p = next(model.parameters())
    return (FUSE_DEBLUR_TRAIN and p.is_cuda and p.dtype == torch.float32 and model.n_feats % 4 == 0
            and all(l.is_cuda and l.device == p.device and l.dtype == torch.float32 and l.dim() == 4 and l.shape[1] in (3, 6)
                    and l.is_contiguous(memory_format=torch.channels_last) and l.numel() > 0 for l in levels))


def _forward_torch(model, levels):
    n = model.n_scales
    out, x = [None] * n, levels[-1][:, :3]
    for s in range(n - 1, -1, -1):
        out[s] = model.body_models[s](x)
        if s > 0:
            x = torch.cat((levels[s - 1][:, :3], model.conv_end_models[s](out[s])), 1)
    return out


def _forward_hip(model, levels):
    def conv(x, m):
        y = F.conv2d(x, m.weight, None, 1, m.padding)
        return y.contiguous(memory_format=torch.channels_last)            # MIOpen's channels-last kernels give this layout already

    n = model.n_scales
    out, x = [None] * n, levels[-1][:, :3]
    for s in range(n - 1, -1, -1):
        body = model.body_models[s].body
        y = _bias_act(conv(x, body[0]), body[0])
        for block in list(body)[1:-1]:
            t = _bias_act(conv(y, block.body[0]), block.body[0], relu=True)
            y = _bias_act(conv(t, block.body[2]), block.body[2], residual=y)
        out[s] = _bias_act(conv(y, body[-1]), body[-1])
        if s > 0:
            up = model.conv_end_models[s].uppath[0]
            x = torch.cat((levels[s - 1][:, :3], F.pixel_shuffle(_bias_act(conv(out[s], up), up), 2)), 1)
            x = x.contiguous(memory_format=torch.channels_last)
    return out


def msresnet_train_forward(model, input_levels):
    """`input_levels`: the levels minus 127.5, finest first, [B, 3, h, w] or [B, 6, h, w] with channels 0..2 holding the level
    (`patch_levels`) -> the list of [B, 3, h, w] outputs of MSResNet before its `+ 127.5`, same order."""
    if len(input_levels) != model.n_scales:
        raise ValueError("%d levels for a network of %d scales" % (len(input_levels), model.n_scales))
    if _hip_ok(model, input_levels):
        out = _forward_hip(model, input_levels)
        model.last_path = "hip"
    else:
        out = _forward_torch(model, input_levels)
        model.last_path = "torch"
    return out


# ---- the loss --------------------------------------------------------------------------------------------------------------------

def l1_level_device(out, target, loss, gscale=1.0):
    """dib_l1_pyramid_loss on one level: `out` channels-last [B, 3, h, w] (or [n_pix, 3]), `target` the same pixels with shape[1] >= 3
    channels of which 0..2 are read; adds the level's mean |out - target| into the 1-element `loss`, returns the gradient."""
    from .. import _lib
    l = _lib.lib()
    n_pix = out.numel() // 3
    grad = torch.empty_like(out)
    work = torch.empty(max(1, l.dib_l1_pyramid_loss_workspace_bytes(n_pix) // 4), dtype=torch.float32, device=out.device)
    _lib.check(l.dib_l1_pyramid_loss(out.data_ptr(), target.data_ptr(), int(target.shape[1]), n_pix, gscale, grad.data_ptr(), loss.data_ptr(),
                                     work.data_ptr(), _lib.stream_of(out)))
    return grad


class _L1Pyramid(torch.autograd.Function):
    """sum over levels of mean |out_s - target_s| as one node: dib_l1_pyramid_loss per level adds into one device scalar and stores
    that level's gradient; the backward scales the stored gradients by the incoming one."""

    @staticmethod
    def forward(ctx, targets, *outs):
        loss = torch.zeros(1, dtype=torch.float32, device=outs[0].device)
        ctx.save_for_backward(*[l1_level_device(o.contiguous(memory_format=torch.channels_last), t, loss) for o, t in zip(outs, targets)])
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad):
        return (None,) + tuple(g * grad for g in ctx.saved_tensors)


def _l1_hip_ok(outputs, targets):
    return (FUSE_DEBLUR_TRAIN and all(o.is_cuda and o.dtype == torch.float32 and o.dim() == 4 and o.shape[1] == 3 and o.numel() > 0
                                      for o in outputs)
            and all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] >= 3 and t.shape[0] == o.shape[0]
                    and t.shape[2:] == o.shape[2:] and t.is_contiguous(memory_format=torch.channels_last) for o, t in zip(outputs, targets)))


def pyramid_l1_loss(outputs, targets):
    """sum_s mean |outputs[s] - targets[s][:, :3]|; both carry the -127.5 shift (`msresnet_train_forward`, `patch_levels`)."""
    if len(outputs) != len(targets):
        raise ValueError("%d outputs, %d targets" % (len(outputs), len(targets)))
    if _l1_hip_ok(outputs, targets):
        return _L1Pyramid.apply(list(targets), *outputs)
    return sum(F.l1_loss(o, t[:, :3]) for o, t in zip(outputs, targets))
