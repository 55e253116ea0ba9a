"""The deblur-first stage: DeepDeblur's multi-scale ResNet in front of the detector (reference engine.py:319-322,
models/deblur/{deblurInterface,MSResNet,ResNet,common,model}.py; `evaluate.py --deblur_first --deblurer_model_location DIR`), the
paper's "deblur, then detect" baseline.  Evaluation only; fp32 unless `--deblur_precision half` (below); `--amp` does not touch it.

What the reference computes on `images_GPU[0]` (blurred, corrupted, still [0, 1]), quirks included:

  1. quantise  q = trunc(x * 255) to 8 bits, the product rounded in the image's own dtype first (Half 0.50195312 -> 128, not 127).
               A value outside [0, 1] is undefined in the reference's uint8 conversion; here q is clamped to 0..255 (NaN -> 0).
  2. pad       bottom and right to a multiple of 2 ** (n_scales - 1), mode "edge".
  3. pyramid   scikit-image's pyramid_gaussian(img, n_scales - 1, multichannel=True) on float32 in 0..255: level 0 is the padded image,
               each further level the previous one smoothed per channel by a separable Gaussian (sigma 2/3, radius 3: seven taps
               exp(-x^2 / (2 sigma^2)), normalised; boundary scipy's "reflect", d c b a | a b c d, periodic when the halo is longer than
               the image; axis 0 first, then axis 1) and halved by an order-1 resize without anti-aliasing -- at a factor of exactly 2 on
               even sizes the mean of each 2 x 2 block.  scikit-image is not a dependency of this project and was not available where
               this was written: this is a STATED READING of it, NOT PINNED against it (tests pin it to scipy.ndimage.gaussian_filter).
  4. network   MSResNet: minus 127.5, coarsest level first through ResNet(in, 3) = conv, n_resblocks x (conv, ReLU, conv, + input),
               conv; conv_end (conv 3 -> 12, PixelShuffle(2)) of a level's output joins the next finer level's input as channels
               3..5; plus 127.5.
  5. finish    crop level 0 to H x W, .add_(0.5).clamp_(0, 255) / 255: no rounding, the half-level bias is the reference's.  The fp32
               [3, H, W] result replaces `images_GPU[0]`.  (On a GPU -- where the reference runs this -- ATen divides a tensor by a
               scalar as a multiplication by the fp32 reciprocal, and so does the kernel; ATen's CPU kernel divides: 1 ulp apart.)

Two ways to the same values, as models/batchnorm.py has them:

  * HIP (include/dib.h: dib_deblur_pyramid / dib_deblur_shuffle_concat / dib_deblur_finish, csrc/dib_deblur.hip): a CUDA Half or fp32
    image and a network with n_feats % 4 == 0.  The image never leaves the device: n_scales launches build every level's
    channels-last input, the convolutions are F.conv2d without bias on channels-last tensors, each followed in place by
    dib_bias_act_nhwc (bias / bias + ReLU / bias + residual); the last convolution's bias of a level is folded into the shuffle
    (coarser levels: after a bias-only pass, since the biased output also feeds conv_end) or into the finish kernel.  Nothing is
    concatenated, nothing synchronises, everything runs on the current stream.
  * torch: everything else (CPU, other shapes), steps 1-5 op for op.  It is what the HIP path is tested against.

`precision="half"` (`--deblur_precision half`) is DeepDeblur's `--precision half` (reference models/deblur/deblurInterface.py:37,40,
52-53): the checkpoint is loaded in fp32, strictly, and the module is then cast to Half; steps 1-3 stay fp32 (the reference builds the
pyramid on the host) and every level is cast to Half; from there every op is a Half op, rounded once, to nearest even:

  4. network   half(half(L) - 127.5); every convolution with its Half bias; ReLU; `res += x` (half(half(conv + b) + x): two roundings);
               PixelShuffle and cat move values; plus 127.5 in Half.  No clamp: beyond 65504 a Half is inf, as in the reference.
  5. finish    the crop, .add_(0.5), .clamp_(0, 255), / 255, each rounded to Half (on a GPU the last is one fp32 product, rounded once).
               The Half [3, H, W] result replaces `images_GPU[0]`, and `deblurImage` returns a Half tensor.

The HIP path then runs the Half forms of the same kernels (dib_deblur_*_f16, dib_bias_act_f16_nhwc behind MIOpen's Half convolutions
without bias; n_feats % 8 == 0), the torch path the same module on `.half()` tensors.  Measured against a float64 run of the stage
(scale 0..1): Half 7.8e-4, fp32 3.6e-7; bf16 would be 3e-3 to 5e-3, a grey level of 255, and is not built.

`last_path` records which of the two ran last ("hip" / "torch"); FUSE_DEBLUR = False forces the torch path on the GPU for A/B runs.
No pretrained DeepDeblur weights ship with this project and nothing is ever downloaded: `write_random_checkpoint` (or
`python -m detectinblur_amd.models.deblur --write_random DIR`) writes a seeded checkpoint in the reference's layout for synthetic runs."""
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

FUSE_DEBLUR = True
RGB_RANGE = 255
SIGMA, RADIUS = 2.0 / 3.0, 3          # skimage's default sigma 2 * downscale / 6; scipy's radius int(4 * sigma + 0.5)


def _conv(cin, cout, k):
    return nn.Conv2d(cin, cout, k, padding=k // 2, bias=True)


class ResBlock(nn.Module):
    def __init__(self, n_feats, k):
        super().__init__()
        self.body = nn.Sequential(_conv(n_feats, n_feats, k), nn.ReLU(True), _conv(n_feats, n_feats, k))

    def forward(self, x):
        return self.body(x) + x


class ResNet(nn.Module):
    def __init__(self, cin, cout, n_feats, k, n_resblocks):
        super().__init__()
        self.body = nn.Sequential(_conv(cin, n_feats, k), *[ResBlock(n_feats, k) for _ in range(n_resblocks)], _conv(n_feats, cout, k))

    def forward(self, x):
        return self.body(x)


class ConvEnd(nn.Module):
    def __init__(self, k):
        super().__init__()
        self.uppath = nn.Sequential(_conv(3, 12, k), nn.PixelShuffle(2))

    def forward(self, x):
        return self.uppath(x)


class MSResNet(nn.Module):
    """state_dict keys and shapes of the reference's MSResNet (`body_models.{s}.body.{i}[.body.{0,2}].{weight,bias}`,
    `conv_end_models.{s}.uppath.0.{weight,bias}` for s >= 1; scale 0 is the finest): a DeepDeblur checkpoint loads strictly.
    forward: a list of [N, 3, h, w] levels in 0..rgb_range, finest first -> the list of outputs, same order and range."""

    def __init__(self, n_scales=3, n_resblocks=19, n_feats=64, kernel_size=5):
        super().__init__()
        self.n_scales, self.n_resblocks, self.n_feats, self.kernel_size = n_scales, n_resblocks, n_feats, kernel_size
        self.mean = RGB_RANGE / 2
        self.body_models = nn.ModuleList([ResNet(6 if s < n_scales - 1 else 3, 3, n_feats, kernel_size, n_resblocks) for s in range(n_scales)])
        self.conv_end_models = nn.ModuleList([None] + [ConvEnd(kernel_size) for _ in range(1, n_scales)])

    @classmethod
    def from_state_dict(cls, state):
        """The architecture is read off the keys and shapes; the weights are loaded strictly."""
        scales = {int(m.group(1)) for m in (re.match(r"body_models\.(\d+)\.", k) for k in state) if m}
        blocks = {int(m.group(1)) for m in (re.match(r"body_models\.0\.body\.(\d+)\.body\.0\.weight$", k) for k in state) if m}
        first = state["body_models.0.body.0.weight"]
        net = cls(n_scales=len(scales), n_resblocks=len(blocks), n_feats=int(first.shape[0]), kernel_size=int(first.shape[-1]))
        net.load_state_dict(state, strict=True)
        return net

    def forward(self, input_pyramid):
        levels = [x - self.mean for x in input_pyramid]
        out = [None] * self.n_scales
        x = levels[-1]
        for s in range(self.n_scales - 1, -1, -1):
            out[s] = self.body_models[s](x)
            if s > 0:
                x = torch.cat((levels[s - 1], self.conv_end_models[s](out[s])), 1)
        return [o + self.mean for o in out]


# ---- steps 1-3 and 5 in plain torch ------------------------------------------------------------------------------------------------

def gauss_taps():
    """scipy.ndimage.gaussian_filter1d's seven weights at sigma 2/3 (float64)."""
    x = np.arange(-RADIUS, RADIUS + 1)
    w = np.exp(-0.5 / (SIGMA * SIGMA) * x ** 2)
    return w / w.sum()


def reflect_indices(n, radius=RADIUS):
    """source index of positions -radius .. n - 1 + radius under scipy's "reflect" (d c b a | a b c d), periodic"""
    i = np.arange(-radius, n + radius) % (2 * n)
    return np.where(i < n, i, 2 * n - 1 - i)


def quantise(image):
    """step 1: [3, H, W] Half or fp32 -> fp32 integers 0..255"""
    q = (image * 255).float()                 # a Half product is rounded to Half here, as in the reference
    return torch.nan_to_num(q, nan=0.0).clamp(0, 255).trunc()


def pad_to_multiple(q, divisor):
    h, w = q.shape[-2:]
    ph, pw = -h % divisor, -w % divisor
    if ph == 0 and pw == 0:
        return q
    rows = torch.arange(h + ph, device=q.device).clamp(max=h - 1)
    cols = torch.arange(w + pw, device=q.device).clamp(max=w - 1)
    return q[..., rows, :][..., cols]


def _smooth_axis(x, axis, taps):
    n = x.shape[axis]
    xp = x.index_select(axis, torch.as_tensor(reflect_indices(n), device=x.device))
    acc = taps[0] * xp.narrow(axis, 0, n)
    for k in range(1, 2 * RADIUS + 1):
        acc = acc + taps[k] * xp.narrow(axis, k, n)
    return acc


def pyramid(q, n_scales):
    """step 3: the padded fp32 [3, Hp, Wp] image -> n_scales levels in 0..255, finest first"""
    taps = [float(np.float32(t)) for t in gauss_taps()]
    levels = [q]
    for _ in range(1, n_scales):
        s = _smooth_axis(_smooth_axis(levels[-1], 1, taps), 2, taps)
        levels.append(0.25 * ((s[:, 0::2, 0::2] + s[:, 0::2, 1::2]) + (s[:, 1::2, 0::2] + s[:, 1::2, 1::2])))
    return levels


def finish(output, H, W):
    """step 5: the network's [1, 3, Hp, Wp] level 0 -> [3, H, W] in [0, 1], in the output's dtype (Half: every op rounds to Half)"""
    return (output[0, :, :H, :W].clone().add_(0.5).clamp_(0, 255) / 255)


# ---- the same steps as HIP launches (csrc/dib_deblur.hip) -----------------------------------------------------------------------

def pyramid_device(image, n_scales, levels=None, dtype=torch.float32):
    """steps 1-3 and the mean shift: a CUDA [3, H, W] Half / fp32 image -> the network's inputs, finest first: channels-last fp32
    [1, 6, Hp >> s, Wp >> s] tensors whose channels 0..2 hold level s minus 127.5 (3..5 are shuffle_concat_device's), the coarsest
    [1, 3, ...].  n_scales launches on the current stream.  `levels`: tensors to write into (tests).
    dtype torch.float16: Half levels holding half(half(level) - 127.5), the pyramid itself computed in fp32 as above (the fp32 copies
    of the levels in between live in a workspace allocated here)."""
    from .. import _lib
    image = image.contiguous()
    H, W = int(image.shape[1]), int(image.shape[2])
    d = 1 << (n_scales - 1)
    Hp, Wp = -(-H // d) * d, -(-W // d) * d
    if levels is None:
        levels = [torch.empty((1, 6 if s < n_scales - 1 else 3, Hp >> s, Wp >> s), dtype=dtype, device=image.device,
                              memory_format=torch.channels_last) for s in range(n_scales)]
    in_dtype = _lib.DIB_F16 if image.dtype == torch.float16 else _lib.DIB_F32
    if levels[0].dtype == torch.float16:
        work = torch.empty(sum(3 * (Hp >> s) * (Wp >> s) for s in range(1, n_scales - 1)), dtype=torch.float32, device=image.device)
        _lib.check(_lib.lib().dib_deblur_pyramid_f16(image.data_ptr(), in_dtype, H, W, n_scales, _lib.ptr_array([t.data_ptr() for t in levels]),
                                                     work.data_ptr() if work.numel() else None, _lib.stream_of(image)))
        return levels
    _lib.check(_lib.lib().dib_deblur_pyramid(image.data_ptr(), in_dtype, H, W, n_scales,
                                             _lib.ptr_array([t.data_ptr() for t in levels]), _lib.stream_of(image)))
    return levels


def shuffle_concat_device(raw, bias, level):
    """conv_end's raw output [1, 12, h, w] (channels-last, no bias) + bias, PixelShuffle(2), into channels 3..5 of `level`
    [1, 6, 2h, 2w] (channels-last), in place of the reference's torch.cat.  Returns `level`.  Both fp32, or both Half (the sum rounded
    to Half; `bias` stays an fp32 vector, of Half values)."""
    from .. import _lib
    h, w = int(raw.shape[2]), int(raw.shape[3])
    assert tuple(raw.shape) == (1, 12, h, w) and tuple(level.shape) == (1, 6, 2 * h, 2 * w)
    assert raw.is_contiguous(memory_format=torch.channels_last) and level.is_contiguous(memory_format=torch.channels_last)
    assert raw.dtype == level.dtype and bias.dtype == torch.float32
    l = _lib.lib()
    fn = l.dib_deblur_shuffle_concat_f16 if raw.dtype == torch.float16 else l.dib_deblur_shuffle_concat
    _lib.check(fn(raw.data_ptr(), bias.data_ptr(), level.data_ptr(), h, w, _lib.stream_of(raw)))
    return level


def finish_device(raw, bias, H, W):
    """step 5 on the finest level's last convolution [1, 3, Hp, Wp] (channels-last, no bias): + bias, + 127.5, + 0.5, clamp, / 255,
    cropped -> planar [3, H, W] of `raw`'s dtype (Half: every one of those ops rounded to Half)"""
    from .. import _lib
    assert raw.shape[0] == 1 and raw.shape[1] == 3 and raw.is_contiguous(memory_format=torch.channels_last)
    assert bias.dtype == torch.float32
    out = torch.empty((3, H, W), dtype=raw.dtype, device=raw.device)
    l = _lib.lib()
    fn = l.dib_deblur_finish_f16 if raw.dtype == torch.float16 else l.dib_deblur_finish
    _lib.check(fn(raw.data_ptr(), bias.data_ptr(), out.data_ptr(), H, W, int(raw.shape[2]), int(raw.shape[3]), _lib.stream_of(raw)))
    return out


# ---- the stage -----------------------------------------------------------------------------------------------------------------------

def find_checkpoint(model_location):
    """`<location>/models/model-<N>.pt`, the file the reference's get_last_epoch picks (the LAST name of sorted(os.listdir): a string
    sort, model-9.pt after model-10.pt), or `model_location` itself when it is a file."""
    if os.path.isfile(model_location):
        return model_location
    save_dir = os.path.join(model_location, "models")
    if not os.path.isdir(save_dir):
        raise FileNotFoundError("--deblurer_model_location %s: neither a checkpoint file nor a directory with models/model-<N>.pt "
                                "(nothing is downloaded; `python -m detectinblur_amd.models.deblur --write_random DIR` writes a random one)"
                                % model_location)
    names = sorted(os.listdir(save_dir))
    if not names:
        raise FileNotFoundError("%s holds no checkpoint" % save_dir)
    epoch = int(re.findall(r"\d+", names[-1])[0])
    return os.path.join(save_dir, "model-%d.pt" % epoch)


PRECISIONS = ("single", "half")            # DeepDeblur's --precision


class Deblurer(nn.Module):
    def __init__(self, model_location, device=None, precision="single"):
        super().__init__()
        if precision not in PRECISIONS:
            raise ValueError("Deblurer(precision=%r): one of %s" % (precision, ", ".join(repr(p) for p in PRECISIONS)))
        self.precision = precision
        self.dtype = torch.float16 if precision == "half" else torch.float32
        self.checkpoint = find_checkpoint(str(model_location))
        print("Loading model from {}".format(self.checkpoint))
        state = torch.load(self.checkpoint, map_location="cpu", weights_only=True)
        self.model = MSResNet.from_state_dict(state["G"]).float()
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.model.to(self.device)
        if self.device.type == "cuda":
            self.model.to(memory_format=torch.channels_last)
        self._bias32 = {}
        if precision == "half":                                            # reference deblurInterface.py:40, after the fp32 load
            self.model.to(dtype=torch.float16)
            if self.device.type == "cuda":
                # the epilogue kernels read per-channel vectors as fp32: the Half biases, upcast (exact)
                self._bias32 = {m: m.bias.detach().float() for m in self.model.modules() if isinstance(m, nn.Conv2d)}
        self.eval()
        for p in self.parameters():
            p.requires_grad_(False)
        self.last_path = None

    @property
    def n_scales(self):
        return self.model.n_scales

    # ---- which path ------------------------------------------------------------------------------------------------------------
    def _hip_ok(self, image):
        return (FUSE_DEBLUR and image.is_cuda and image.dim() == 3 and image.shape[0] == 3 and image.numel() > 0
                and image.dtype in (torch.float16, torch.float32) and self.model.n_feats % (8 if self.precision == "half" else 4) == 0
                and 1 <= self.n_scales <= 4
                and next(self.model.parameters()).device == image.device)

    # ---- the torch path --------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _network_torch(self, q, H, W):
        """q: fp32 [3, H, W] integers 0..255 -> the network's level 0, cropped: [1, 3, H, W] in 0..255, fp32 or (precision half) Half:
        the fp32 pyramid cast to the module's dtype, as the reference's dataCommon.to does"""
        levels = pyramid(pad_to_multiple(q, 2 ** (self.n_scales - 1)), self.n_scales)
        return self.model([l[None].to(self.dtype) for l in levels])[0][:, :, :H, :W]

    @torch.no_grad()
    def deblurImage(self, image):
        """The reference's method: an H x W x 3 uint8 array -> the [1, 3, H, W] fp32 (precision half: Half) tensor in 0..255 on the deblurrer's device,
        BEFORE the finish step (the caller applies `.add_(0.5).clamp_(0, 255) / 255`).  Always the torch path."""
        q = torch.from_numpy(np.ascontiguousarray(np.asarray(image))).to(self.device).permute(2, 0, 1).float()
        self.last_path = "torch"
        return self._network_torch(q, q.shape[1], q.shape[2]).contiguous()

    @torch.no_grad()
    def _deblur_torch(self, image):
        image = image.to(self.device)
        H, W = image.shape[-2:]
        self.last_path = "torch"
        return finish(self._network_torch(quantise(image), H, W), H, W)

    # ---- the HIP path ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _deblur_hip(self, image):
        from .. import _lib
        l, n = _lib.lib(), self.n_scales
        H, W = int(image.shape[1]), int(image.shape[2])
        half = self.precision == "half"
        levels = pyramid_device(image, n, dtype=self.dtype)
        stream = _lib.stream_of(image)
        epilogue = l.dib_bias_act_f16_nhwc if half else l.dib_bias_act_nhwc
        bias_of = (lambda m: self._bias32[m]) if half else (lambda m: m.bias)

        def conv(x, m):
            y = F.conv2d(x, m.weight, None, 1, m.padding)
            return y.contiguous(memory_format=torch.channels_last)        # MIOpen's channels-last kernels give this layout already

        def bias_act(y, bias, residual=None, relu=False):
            _lib.check(epilogue(y.data_ptr(), bias.data_ptr(), residual.data_ptr() if residual is not None else None, y.numel(),
                                y.shape[1], int(relu), stream))
            return y

        out, x = None, levels[n - 1]
        for s in range(n - 1, -1, -1):
            body = self.model.body_models[s].body
            y = bias_act(conv(x, body[0]), bias_of(body[0]))
            for block in list(body)[1:-1]:
                t = bias_act(conv(y, block.body[0]), bias_of(block.body[0]), relu=True)
                y = bias_act(conv(t, block.body[2]), bias_of(block.body[2]), residual=y)
            z = conv(y, body[-1])                                          # raw: its bias goes into the kernel that reads it
            if s > 0:
                up = self.model.conv_end_models[s].uppath[0]
                x = shuffle_concat_device(conv(bias_act(z, bias_of(body[-1])), up), bias_of(up), levels[s - 1])
            else:
                out = finish_device(z, bias_of(body[-1]), H, W)
        self.last_path = "hip"
        return out

    # ---- entry point -----------------------------------------------------------------------------------------------------------
    def deblur_(self, image):
        """[3, H, W] Half or fp32 in [0, 1] -> fp32 (precision half: Half) [3, H, W] in [0, 1] on the same device: steps 1-5."""
        if image.dim() != 3 or image.shape[0] != 3:
            raise ValueError("deblur_ expects a [3, H, W] image, got {}".format(tuple(image.shape)))
        if self._hip_ok(image):
            return self._deblur_hip(image)
        return self._deblur_torch(image)

    forward = deblur_


def write_random_checkpoint(directory, n_feats=64, n_resblocks=19, n_scales=3, kernel_size=5, seed=0, epoch=1):
    """A seeded random MSResNet as `<directory>/models/model-<epoch>.pt` holding {"G": state_dict}: the reference's layout.  Weights are
    uniform in +-1 / sqrt(fan_in), biases in +-0.05: a convolution passes a third of its input's power on, so 2 x 19 of them in residual
    blocks neither die out nor saturate and the output stays inside 0..255."""
    g = torch.Generator().manual_seed(seed)
    net = MSResNet(n_scales=n_scales, n_resblocks=n_resblocks, n_feats=n_feats, kernel_size=kernel_size)
    with torch.no_grad():
        for p in net.parameters():
            fan_in = p[0].numel() if p.dim() == 4 else 1
            bound = 1.0 / math.sqrt(fan_in) if p.dim() == 4 else 0.05
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * bound)
    path = os.path.join(str(directory), "models", "model-%d.pt" % epoch)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save({"G": net.state_dict()}, path)
    return path


def _main():
    import argparse
    p = argparse.ArgumentParser(description="writes a random DeepDeblur checkpoint in the reference's layout (synthetic runs, tests)")
    p.add_argument("--write_random", required=True, metavar="DIR")
    p.add_argument("--n_feats", type=int, default=64)
    p.add_argument("--n_resblocks", type=int, default=19)
    p.add_argument("--n_scales", type=int, default=3)
    p.add_argument("--kernel_size", type=int, default=5)
    p.add_argument("--seed", type=int, default=0)
    a = p.parse_args()
    print(write_random_checkpoint(a.write_random, a.n_feats, a.n_resblocks, a.n_scales, a.kernel_size, a.seed))


if __name__ == "__main__":
    _main()
