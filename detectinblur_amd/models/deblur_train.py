"""The training path of DeepDeblur's MSResNet (models/deblur.py holds the network and the inference stage; this file leaves both as
they are).  The reference vendors DeepDeblur's trainer beside the inference wrapper (models/deblur/train.py, dataCommon.py,
model.py); `python -m detectinblur_amd.train_deblurrer` is this project's, fed by the GPU blur.  What is here:

  draws     `draw_patch`: one patch origin and one augmentation per image from Python's `random`, in the order of the reference's
            dataCommon.py -- crop (:32-33) draws randrange for py, then for px; augment (:61-68) draws choice for hflip, for vflip and
            for rot90, then shuffles the channel order.  The patch is cropped first, then hflip (reverse x), vflip (reverse y),
            rot90 (a transpose), then the channel order (:76-81).  On request, then from `np.random` as the reference does: the
            saturation factor uniform(0.5, 1.5) (:73), add_noise's sigma normal() * sigma_sigma (:48), and two 32-bit key words that
            stand in for its randn field (:51).  With neither asked for, no generator sees an extra draw.
  patches   `gather_patches`: the patches of a ragged list of images as one planar [B, 3, ps, ps] tensor: dib_deblur_patches on the
            GPU (one launch, bit-exact data movement), `gather_patches_torch` elsewhere and as the reference of the tests.
  values    `augment_patches`: the same patches with dataCommon's HSV saturation change (:83-87) and add_noise (:50-52) applied, as
            fp32 grey levels / 255: dib_deblur_patches_augment on the GPU (one launch per list), `augment_patches_torch` elsewhere.
            Scaling S in HSV and converting back has a closed form without the hue, x_c = clip(m - a (m - q_c), 0, 255) with m the
            pixel's maximum (csrc/dib_deblur_augment.hip states the four steps), so no colour conversion is needed.  Two stated
            readings: the patch is quantised to 8 bits first (the reference's `augment` runs on the uint8 array of an image file),
            and the result is rounded to the nearest grey level, where the reference hands unrounded floats to its pyramid: at most
            half a level, against a sigma of typically 2.
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
            MIXED PRECISION (`--amp`; the reference's train.py:43-46, 97-103): Half levels (`patch_levels(..., torch.float16)`) into
            the fp32 parameters give Half outputs, again two ways ("hip-amp" / "torch-amp"):
              * HIP: as above with n_feats % 8 == 0 and FUSE_DEBLUR_TRAIN_AMP.  F.conv2d on Half tensors with `weight.to(float16)` --
                autograd's own cast, so the master weights get fp32 gradients -- each followed in place by dib_bias_act_f16_nhwc, or
                dib_bias_act_mask_f16_nhwc for the ReLU, with the fp32 master bias (`_BiasActTrainHalf`); the backward is one
                dib_bias_grad_f16_nhwc: Half gradient through, fp32 bias gradient.  The 3- and 12-channel convolutions take the
                scalar epilogue and one channel per lane.  `forward_amp_restated` states its arithmetic in torch ops (tests).
              * torch: the plain module under torch.autocast(dtype=float16), the reference's.
  loss      `pyramid_l1_loss`: sum over levels of mean |output - target| (DeepDeblur's published L1 loss; its loss/ package is not in
            the reference tree: a stated reading).  On the HIP path one autograd node: dib_l1_pyramid_loss per level adds the level's
            mean into one device scalar and stores the gradient, the backward scales it by the incoming gradient.  The gradient is
            sign(d) / (3 n_pix) with sign(+-0) = 0; a NaN difference gives a NaN gradient there, where torch.sign -- and with it the
            plain path's l1_loss backward -- gives 0: the loss is NaN on both paths, and the driver stops at its next read of it.
            Under --amp there is no Half loss kernel (three 3-channel outputs are 0.03 % of the step): each Half output goes through
            `.float()` into this loss, so the loss read is the true, unscaled fp32 loss; GradScaler's `scale(loss).backward()`
            multiplies the stored sign(d) * k by the scale in fp32 and the cast's backward rounds it to Half once.  The one thing the
            scaler cannot see: that product, scale / (3 n_pix), has to stay above Half's subnormal range (2^-14 = 6.1e-5) or the
            gradient of a level loses bits, or all of them, without an inf to skip the step on: 3.3e-4 at the defaults (level 0:
            n_pix = 16 x 256 x 256) with scale 1024; GradScaler halves the scale on an overflow and never looks below.

Summation order and the depth of its tree (for error bounds): csrc/dib_sliced_sum.h; restated below as `bias_grad_depth` and
`sliced_sum_depth`.  models/deblur_adversarial.py takes from here what its discriminator and loss share with the generator's: `lanes`,
`mask_bits_torch`, `nhwc_grad`, `sliced_sum_depth`, `choose_path` and `stored_grad_sum`."""
import collections
import ctypes
import math
import random

import numpy as np
import torch
import torch.nn.functional as F

from . import deblur

# False: the plain module on the GPU too, for A/B runs.  On: 292.0 against 300.7 ms per step at the trainer's defaults on an MI355X,
# alternated, spread 0.3 % (profiles/deblur_train.txt).
FUSE_DEBLUR_TRAIN = True
# The same decision for the Half epilogues under --amp, which run only where FUSE_DEBLUR_TRAIN is on as well; False: the plain module
# under torch.autocast.  On: 97.2 against 103.1 ms per step at the trainer's defaults, alternated, spread 0.3 %; fp32 in the same run:
# 289.4 ms (profiles/deblur_train_amp.txt).
FUSE_DEBLUR_TRAIN_AMP = True

PATCH_HFLIP, PATCH_VFLIP, PATCH_ROT90 = 1, 2, 4          # include/dib.h DIB_PATCH_*
PATCH_MAX_BATCH = 64                                     # images per dib_deblur_patches launch

# saturation: augment's amp_factor; sigma: add_noise's, in grey levels (it may be negative: a normal draw); key: the noise field's
PatchDraw = collections.namedtuple("PatchDraw", "py px hflip vflip rot90 order saturation sigma key", defaults=(1.0, 0.0, (0, 0)))


# ---- draws -----------------------------------------------------------------------------------------------------------------------

def draw_patch(h, w, ps, change_saturation=False, noise_sigma=0.0):
    """One image's draws, in dataCommon.py's order (crop :32-33, augment :61-68), from Python's `random`; then, only when asked for,
    from `np.random` as the reference draws them: augment's amp_factor (:73), add_noise's sigma (:48, sigma_sigma = `noise_sigma`,
    rgb_range = 255) and two 32-bit words, the key of the noise field that stands in for its randn (:51)."""
    py = random.randrange(0, h - ps + 1)
    px = random.randrange(0, w - ps + 1)
    choices = (False, True)
    hflip = random.choice(choices)
    vflip = random.choice(choices)
    rot90 = random.choice(choices)
    order = list(range(3))
    random.shuffle(order)
    draw = PatchDraw(py, px, hflip, vflip, rot90, tuple(order))
    if change_saturation:
        draw = draw._replace(saturation=float(np.random.uniform(0.5, 1.5)))
    if noise_sigma:
        sigma = float(np.random.normal() * noise_sigma)
        key = np.random.randint(0, 2 ** 32, size=2, dtype=np.uint32)
        draw = draw._replace(sigma=sigma, key=(int(key[0]), int(key[1])))
    return draw


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


def _patch_chunks(who, images, draws):
    """What both patch entry points take per image: checks the images, then for each run of at most PATCH_MAX_BATCH of them yields
    (first index, draws, the leading arguments of the call: pointers, dtype, H, W, py, px, flags)."""
    from .. import _lib
    first = images[0]
    if first.dtype not in (torch.float16, torch.float32) or any(im.dtype != first.dtype or im.device != first.device or im.dim() != 3
                                                                  or im.shape[0] != 3 for im in images):
        raise ValueError("%s: planar [3, H, W] Half or fp32 images of one dtype on one device" % who)
    images = [im.contiguous() for im in images]
    dtype = _lib.DIB_F16 if first.dtype == torch.float16 else _lib.DIB_F32
    for b0 in range(0, len(images), PATCH_MAX_BATCH):
        ims, ds = images[b0:b0 + PATCH_MAX_BATCH], draws[b0:b0 + PATCH_MAX_BATCH]
        yield b0, ds, (_lib.ptr_array([im.data_ptr() for im in ims]), dtype, _lib.int_array([int(im.shape[1]) for im in ims]),
                       _lib.int_array([int(im.shape[2]) for im in ims]), _lib.int_array([d.py for d in ds]),
                       _lib.int_array([d.px for d in ds]), (ctypes.c_uint * len(ds))(*[flags_word(d) for d in ds]))


def gather_patches_device(images, draws, ps):
    from .. import _lib
    out = torch.empty((len(images), 3, ps, ps), dtype=images[0].dtype, device=images[0].device)
    for b0, ds, args in _patch_chunks("gather_patches", images, draws):
        _lib.check(_lib.lib().dib_deblur_patches(*args, len(ds), ps, out[b0].data_ptr(), _lib.stream_of(out)))
    return out


def gather_patches(images, draws, ps):
    if images[0].is_cuda:
        return gather_patches_device(images, draws, ps)
    return gather_patches_torch(images, draws, ps)


# ---- patches with the saturation change and the noise ----------------------------------------------------------------------------

def noise_seed(key):
    """The seed `augment_patches_torch` gives its torch.Generator for a draw's key.  torch's CPU generator reads the low 32 bits of a
    seed only, so both words are mixed into those."""
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    return (k1 << 32) | (k0 ^ ((k1 * 0x9E3779B1) & 0xFFFFFFFF))


def augment_patches_torch(images, draws, ps, noise, pre_rounding=False):
    """planar [3, H_b, W_b] Half or fp32 images -> fp32 [B, 3, ps, ps]: `gather_patches_torch`, then csrc/dib_deblur_augment.hip's four
    steps op for op in torch fp32 on the 0..255 scale -- quantise; x = clip(m - a (m - q), 0, 255) with m the pixel's maximum;
    with `noise` and a sigma other than 0, x = clip(x + sigma n, 0, 255); round to the nearest level, / 255.  On a GPU it is bit-equal to
    the kernel whenever sigma == 0.  THE NOISE FIELD n is torch.randn from a CPU torch.Generator seeded with the draw's key
    (`noise_seed`): the kernel's field (Philox + Box-Muller on the element index) in distribution, NOT in bits.
    pre_rounding (tests): the values before the last step, on the 0..255 scale."""
    out = []
    for img, d in zip(images, draws):
        p = gather_patches_torch([img], [d], ps)[0]
        q = deblur.quantise(p) + 0.0                      # (+ 0.0: a -0.0 that clamp may let through becomes the kernel's +0.0)
        m = q.amax(0, keepdim=True)
        t = (m - q) * float(np.float32(d.saturation))     # an exact integer times the fp32 factor: one rounding
        x = (m - t).clamp(0, 255)
        if noise and d.sigma != 0:
            g = torch.Generator().manual_seed(noise_seed(d.key))
            n = torch.randn((3, ps, ps), generator=g, dtype=torch.float32).to(x.device)
            x = (x + n * float(np.float32(d.sigma))).clamp(0, 255)
        # a true division: by a Python scalar, torch on a GPU multiplies by the rounded reciprocal instead
        out.append(x if pre_rounding else x.round() / torch.full((), 255.0, dtype=torch.float32, device=x.device))
    return torch.stack(out).contiguous()


def augment_patches_device(images, draws, ps, noise):
    from .. import _lib
    out = torch.empty((len(images), 3, ps, ps), dtype=torch.float32, device=images[0].device)
    for b0, ds, args in _patch_chunks("augment_patches", images, draws):
        n = len(ds)
        saturation = (ctypes.c_float * n)(*[d.saturation for d in ds])
        sigma = (ctypes.c_float * n)(*[d.sigma if noise else 0.0 for d in ds])
        keys = (ctypes.c_uint * (2 * n))(*[int(k) & 0xFFFFFFFF for d in ds for k in d.key])
        _lib.check(_lib.lib().dib_deblur_patches_augment(*args, saturation, sigma, keys, n, ps, out[b0].data_ptr(), _lib.stream_of(out)))
    return out


def augment_patches(images, draws, ps, noise):
    """The patches of `gather_patches` with each draw's saturation change and, with `noise` (the blurred input; the sharp target
    passes False), its noise: fp32 [B, 3, ps, ps] holding grey levels / 255, ready for `patch_levels`."""
    if images[0].is_cuda:
        return augment_patches_device(images, draws, ps, noise)
    return augment_patches_torch(images, draws, ps, noise)


# ---- pyramid ---------------------------------------------------------------------------------------------------------------------

def _level_shape(B, ps, s, n_scales):
    return (B, 6 if s < n_scales - 1 else 3, ps >> s, ps >> s)


def patch_levels(patches, n_scales, dtype=torch.float32):
    """[B, 3, ps, ps] Half or fp32 in [0, 1] (ps a multiple of 2 ** (n_scales - 1)) -> the levels minus 127.5, finest first, as
    channels-last fp32 [B, 6, ps >> s, ps >> s] tensors (coarsest [B, 3, ...]) of which channels 0..2 are written.
    dtype torch.float16 (the inputs under --amp): Half tensors of the same shapes -- dib_deblur_pyramid_f16's half(half(level) - 127.5)
    on the GPU (the pyramid itself is computed in fp32), the cast of the fp32 levels elsewhere."""
    if dtype not in (torch.float32, torch.float16):
        raise ValueError("patch_levels: fp32 or Half levels")
    B, ps = int(patches.shape[0]), int(patches.shape[-1])
    if ps % (1 << (n_scales - 1)):
        raise ValueError("patch size %d is not a multiple of %d" % (ps, 1 << (n_scales - 1)))
    elem = 2 if dtype == torch.float16 else 4
    # the pyramid kernels want every slab on 16 bytes: 12 (ps >> s)^2 bytes per fp32 patch at the coarsest level
    device_ok = patches.is_cuda and 1 <= n_scales <= 4 and all(math.prod(_level_shape(1, ps, s, n_scales)) * elem % 16 == 0 for s in range(n_scales))
    if dtype == torch.float16 and not device_ok:
        return [l.to(dtype) for l in patch_levels(patches, n_scales)]
    levels = [torch.empty(_level_shape(B, ps, s, n_scales), dtype=dtype, device=patches.device, memory_format=torch.channels_last)
              for s in range(n_scales)]
    if device_ok:
        from .. import _lib
        patches = patches.contiguous()
        l, stream = _lib.lib(), _lib.stream_of(patches)
        in_dtype = _lib.DIB_F16 if patches.dtype == torch.float16 else _lib.DIB_F32
        if dtype == torch.float16:
            # the fp32 copies of the levels between the finest and the coarsest (include/dib.h): one workspace for all B calls, which
            # run one after the other on the stream
            work = torch.empty(sum(3 * (ps >> s) ** 2 for s in range(1, n_scales - 1)), dtype=torch.float32, device=patches.device)
            work_ptr = work.data_ptr() if work.numel() else None
        for b in range(B):
            ptrs = _lib.ptr_array([t[b].data_ptr() for t in levels])
            if dtype == torch.float16:
                _lib.check(l.dib_deblur_pyramid_f16(patches[b].data_ptr(), in_dtype, ps, ps, n_scales, ptrs, work_ptr, stream))
            else:
                _lib.check(l.dib_deblur_pyramid(patches[b].data_ptr(), in_dtype, ps, ps, n_scales, ptrs, stream))
        return levels
    for b in range(B):
        for l, v in zip(levels, deblur.pyramid(deblur.quantise(patches[b]), n_scales)):
            l[b, :3] = v - deblur.RGB_RANGE / 2
    return levels


# ---- the epilogue with its one-pass backward ---------------------------------------------------------------------------------------

def _ceil_div(a, b):
    return -(-a // b)


def bias_grad_depth(n_pix, C, V=None):
    """Additions any one input of dib_bias_grad_nhwc's channel sum can pass through (csrc/dib_sliced_sum.h, "THE SUMMATION ORDER").
    V: channels per lane; None is the fp32 form's (4 when C % 4 == 0, else 1).  dib_bias_grad_f16_nhwc on 16-byte aligned gradients:
    `bias_grad_lanes(C, torch.float16)`, 8 when C % 8 == 0, else 1."""
    if V is None:
        V = 4 if C % 4 == 0 else 1
    if V not in (1, 4, 8) or C % V:
        raise ValueError("bias_grad_depth: V = %r with C = %d" % (V, C))
    QB = min(C // V, 256)
    R = 256 // QB
    S = max(1, min(1024, _ceil_div(n_pix, 16 * R)))
    L = _ceil_div(_ceil_div(n_pix, S), R)
    return L + (R - 1).bit_length() + S - 1


def sliced_sum_depth(n):
    """The same for a scalar loss over n elements (csrc/dib_sliced_sum.h, "scalar losses"); the division and the addition onto the
    scalar come on top."""
    S = max(1, min(1024, _ceil_div(n, 2048)))
    return _ceil_div(_ceil_div(n, S), 256) + 8 + S - 1


def l1_loss_depth(n_pix):
    """dib_l1_pyramid_loss's sum of |d|"""
    return sliced_sum_depth(3 * n_pix)


def lanes(dtype):
    """Elements of a 16-byte lane, and with that per mask byte: 8 Half, 4 fp32."""
    return 8 if dtype == torch.float16 else 4


def bias_grad_lanes(C, dtype):
    """Channels per lane of the bias-gradient kernels on 16-byte aligned gradients."""
    return lanes(dtype) if C % lanes(dtype) == 0 else 1


def sign_mask_torch(y):
    """dib_bias_act_mask_nhwc's mask of a [n_pix, C] (C % 4 == 0) tensor: one byte per 4 consecutive elements, bit k = element > 0.
    A Half `y` (C % 8 == 0): dib_bias_act_mask_f16_nhwc's, one byte per 8."""
    bits = (y.reshape(-1, lanes(y.dtype)) > 0).to(torch.uint8)
    mask = bits[:, 0]
    for k in range(1, bits.shape[1]):
        mask = mask | (bits[:, k] << k)
    return mask


def mask_bits_torch(mask, like):
    """The bytes of `sign_mask_torch` back as one bool per element of `like`."""
    shifts = torch.arange(lanes(like.dtype), device=mask.device, dtype=torch.uint8)
    return ((mask.reshape(-1, 1) >> shifts) & 1).reshape(like.shape).bool()


def bias_grad_torch(grad, mask=None):
    """dib_bias_grad_nhwc restated: grad [n_pix, C] -> (grad_out, bias_grad).  A Half `grad`: dib_bias_grad_f16_nhwc, with its mask
    of one byte per 8 elements, a Half grad_out and the fp32 sum of the upcast values."""
    if mask is not None:
        grad = torch.where(mask_bits_torch(mask, grad), grad, torch.zeros((), dtype=grad.dtype, device=grad.device))
    return grad, (grad.float() if grad.dtype == torch.float16 else grad).sum(0)


def l1_level_torch(out, target, gscale=1.0):
    """dib_l1_pyramid_loss restated: out [n_pix, 3], target [n_pix, >= 3] -> (grad, the level's addend to the loss)."""
    d = out - target[:, :3]
    n = torch.tensor(float(out.numel()), dtype=out.dtype)
    k = (torch.tensor(gscale, dtype=out.dtype) / n).to(out.device)
    grad = torch.where(torch.isnan(d), d, torch.sign(d) * k)
    return grad, d.abs().sum() / n.to(out.device)


def bias_grad_device(grad, mask=None, out=None):
    """dib_bias_grad_nhwc on a channels-last [N, C, H, W] (or a [n_pix, C]) fp32 gradient -> (grad_out, bias_grad); `out` may be
    `grad` itself; without a mask nothing is written and `grad` is returned as it came.  A Half gradient: dib_bias_grad_f16_nhwc
    (grad_out Half, bias_grad fp32)."""
    from .. import _lib
    C = int(grad.shape[1])
    n_pix = grad.numel() // C
    l = _lib.lib()
    half = grad.dtype == torch.float16
    size, run = (l.dib_bias_grad_f16_workspace_bytes, l.dib_bias_grad_f16_nhwc) if half else (l.dib_bias_grad_workspace_bytes, l.dib_bias_grad_nhwc)
    bias_grad = torch.empty(C, dtype=torch.float32, device=grad.device)
    work = torch.empty(max(1, size(n_pix, C) // 4), dtype=torch.float32, device=grad.device)
    if mask is not None and out is None:
        out = torch.empty_like(grad)
    _lib.check(run(grad.data_ptr(), mask.data_ptr() if mask is not None else None, out.data_ptr() if out is not None else None,
                   n_pix, C, bias_grad.data_ptr(), work.data_ptr(), _lib.stream_of(grad)))
    return (out if out is not None else grad), bias_grad


def _bias_act_forward(ctx, x, bias, residual, relu, act, act_mask, lane):
    """The forward of both epilogue nodes: entry points `act` / `act_mask` (with the ReLU: one mask byte per `lane` elements)."""
    from .. import _lib
    C = int(x.shape[1])
    res = residual.data_ptr() if residual is not None else None
    ctx.has_res, ctx.masked = residual is not None, bool(relu)
    l, stream = _lib.lib(), _lib.stream_of(x)
    if relu:
        mask = torch.empty(x.numel() // lane, dtype=torch.uint8, device=x.device)
        _lib.check(getattr(l, act_mask)(x.data_ptr(), bias.data_ptr(), res, x.numel(), C, mask.data_ptr(), stream))
        ctx.save_for_backward(mask)
    else:
        _lib.check(getattr(l, act)(x.data_ptr(), bias.data_ptr(), res, x.numel(), C, 0, stream))
    ctx.mark_dirty(x)
    return x


def nhwc_grad(grad):
    """An incoming gradient as the one-launch backwards take it: in NHWC element order (the mask's and the channel index's) and on 16
    bytes.  They never write it in place: autograd may hand the same gradient tensor to another node."""
    if not grad.is_contiguous(memory_format=torch.channels_last):
        grad = grad.contiguous(memory_format=torch.channels_last)
    if grad.data_ptr() & 15:
        grad = grad.clone(memory_format=torch.channels_last)
    return grad


class _BiasActTrain(torch.autograd.Function):
    """x = act(x + bias[c] (+ residual)) in place on a channels-last fp32 CUDA convolution output (dib_bias_act_nhwc, or
    dib_bias_act_mask_nhwc with the ReLU); the backward is one launch pair over the gradient (dib_bias_grad_nhwc): masked gradient and
    bias gradient from the same read.  Modelled on the trunk's `_BiasAct` (models/backbone.py), which keeps torch's separate sum."""

    @staticmethod
    def forward(ctx, x, bias, residual, relu):
        return _bias_act_forward(ctx, x, bias, residual, relu, "dib_bias_act_nhwc", "dib_bias_act_mask_nhwc", 4)

    @staticmethod
    def backward(ctx, grad):
        grad, gb = bias_grad_device(nhwc_grad(grad), ctx.saved_tensors[0] if ctx.masked else None)
        return grad, gb, (grad if ctx.has_res else None), None


class _BiasActTrainHalf(_BiasActTrain):
    """Its Half twin (--amp): in place on a channels-last Half CUDA convolution output with the fp32 master bias, which is never
    rounded to Half -- dib_bias_act_f16_nhwc (8 channels per lane, or its scalar form for the 3- and 12-channel convolutions), or
    dib_bias_act_mask_f16_nhwc with the ReLU (C % 8 == 0).  The inherited backward is one dib_bias_grad_f16_nhwc: the Half gradient
    masked bit for bit, the bias gradient summed in fp32."""

    @staticmethod
    def forward(ctx, x, bias, residual, relu):
        return _bias_act_forward(ctx, x, bias, residual, relu, "dib_bias_act_f16_nhwc", "dib_bias_act_mask_f16_nhwc", 8)


def _bias_act(y, conv, residual=None, relu=False):
    return (_BiasActTrainHalf if y.dtype == torch.float16 else _BiasActTrain).apply(y, conv.bias, residual, relu)


# ---- the network -----------------------------------------------------------------------------------------------------------------

def _hip_ok(model, levels, dtype=torch.float32):
    """`dtype`: of the levels (the parameters are fp32 either way); Half lanes hold 8 channels."""
    p = next(model.parameters())
    return (FUSE_DEBLUR_TRAIN and (FUSE_DEBLUR_TRAIN_AMP or dtype != torch.float16) and p.is_cuda and p.dtype == torch.float32
            and model.n_feats % lanes(dtype) == 0
            and all(l.is_cuda and l.device == p.device and l.dtype == dtype and l.dim() == 4 and l.shape[1] in (3, 6)
                    and l.is_contiguous(memory_format=torch.channels_last) and l.numel() > 0 for l in levels))


def _amp(model, levels):
    """Half levels into fp32 parameters: the mixed-precision step (--amp)."""
    return next(model.parameters()).dtype == torch.float32 and len(levels) > 0 and all(l.dtype == torch.float16 for l in levels)


def _forward_torch(model, levels):
    n = model.n_scales
    out, x = [None] * n, levels[-1][:, :3]
    for s in range(n - 1, -1, -1):
        out[s] = model.body_models[s](x)
        if s > 0:
            x = torch.cat((levels[s - 1][:, :3], model.conv_end_models[s](out[s])), 1)
    return out


def forward_amp_restated(model, levels):
    """TEST ONLY: the arithmetic of the HIP path under --amp in torch ops on explicit Half tensors -- the same F.conv2d calls, the bias
    added to the upcast output and rounded once, the ReLU on Half, the residual added to the upcast values and rounded again."""
    def conv(x, m, residual=None, relu=False):
        y = F.conv2d(x, m.weight.to(torch.float16), None, 1, m.padding).contiguous(memory_format=torch.channels_last)
        y = (y.float() + m.bias.view(1, -1, 1, 1)).half()
        if residual is not None:
            y = (y.float() + residual.float()).half()
        return F.relu(y) if relu else y

    n = model.n_scales
    out, x = [None] * n, levels[-1][:, :3]
    for s in range(n - 1, -1, -1):
        body = model.body_models[s].body
        y = conv(x, body[0])
        for block in list(body)[1:-1]:
            y = conv(conv(y, block.body[0], relu=True), block.body[2], residual=y)
        out[s] = conv(y, body[-1])
        if s > 0:
            up = model.conv_end_models[s].uppath[0]
            x = torch.cat((levels[s - 1][:, :3], F.pixel_shuffle(conv(out[s], up), 2)), 1).contiguous(memory_format=torch.channels_last)
    return out


def _forward_hip(model, levels):
    half = levels[0].dtype == torch.float16

    def conv(x, m):
        # --amp: the cast is autograd's own, so the fp32 master weight gets an fp32 gradient
        y = F.conv2d(x, m.weight.to(torch.float16) if half else m.weight, None, 1, m.padding)
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


def choose_path(module, amp, hip_ok, hip_fn, torch_fn):
    """The output of `hip_fn()` where `hip_ok`, else of `torch_fn()` -- with `amp`, the reference's mixed-precision forward
    (models/deblur/train.py:97-99): the plain module under autocast.  `module.last_path` records which: "hip" / "torch", with
    `amp` "hip-amp" / "torch-amp"."""
    if hip_ok:
        out = hip_fn()
    elif amp:
        with torch.autocast(next(module.parameters()).device.type, dtype=torch.float16):
            out = torch_fn()
    else:
        out = torch_fn()
    module.last_path = ("hip" if hip_ok else "torch") + ("-amp" if amp else "")
    return out


def msresnet_train_forward(model, input_levels):
    """`input_levels`: the levels minus 127.5, finest first, [B, 3, h, w] or [B, 6, h, w] with channels 0..2 holding the level
    (`patch_levels`) -> the list of [B, 3, h, w] outputs of MSResNet before its `+ 127.5`, same order.  Half levels into fp32
    parameters (--amp): Half outputs; the caller takes the loss on their `.float()`."""
    if len(input_levels) != model.n_scales:
        raise ValueError("%d levels for a network of %d scales" % (len(input_levels), model.n_scales))
    amp = _amp(model, input_levels)
    return choose_path(model, amp, _hip_ok(model, input_levels, torch.float16 if amp else torch.float32),
                       lambda: _forward_hip(model, input_levels), lambda: _forward_torch(model, input_levels))


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


class _StoredGradSum(torch.autograd.Function):
    """A sum of terms as one node: `term(x, item, loss)` adds the term of tensor x (with its target, or its label) into the 1-element
    `loss` and returns d term / d x, which is stored; the backward scales the stored gradients by the incoming one."""

    @staticmethod
    def forward(ctx, term, items, *tensors):
        loss = torch.zeros(1, dtype=tensors[0].dtype, device=tensors[0].device)
        ctx.save_for_backward(*[term(x, item, loss) for x, item in zip(tensors, items)])
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad):
        return (None, None) + tuple(g * grad for g in ctx.saved_tensors)


def stored_grad_sum(term, tensors, items):
    return _StoredGradSum.apply(term, list(items), *tensors)


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
        # dib_l1_pyramid_loss per level: one device scalar for all levels
        return stored_grad_sum(lambda o, t, loss: l1_level_device(o.contiguous(memory_format=torch.channels_last), t, loss), outputs, targets)
    return sum(F.l1_loss(o, t[:, :3]) for o, t in zip(outputs, targets))
