"""DeepDeblur's adversarial loss for the trainer (`train_deblurrer.py --loss 1*L1+1*ADV`; models/deblur_train.py holds the generator's
training path and leaves this file's names alone).  The reference vendors the network (models/deblur/discriminator.py), builds it
whenever --loss contains `adv` (model.py:31-34) and saves it as "D" beside "G"; DeepDeblur's loss/ package, which holds the loss
itself, is not in the reference tree: binary cross-entropy with logits against the labels real = 1, fake = 0 is a STATED READING
(train_deblurrer.py, "One step with ADV").  What is here:

  network   `Discriminator(n_feats, kernel_size)`: the reference's state-dict keys (conv_layers.0.weight .. conv_layers.9.weight,
            dense.weight; no biases), ten convolutions each followed by LeakyReLU(0.2), strides 1 2 1 2 1 4 1 4 1 and a last 4 x 4
            convolution of stride 4 without padding, then a 1 x 1 convolution to one logit per remaining position.  A 5 x 5 layer of
            stride s maps n to ceil(n / s), the last layer needs 4, so THE SMALLER SIDE MUST BE AT LEAST 193 (`min_side`).
  forward   `discriminator_forward(D, x)`, x [B, 3, H, W] fp32 or Half on the 0..255 scale.  Two ways to the same values, as in
            models/deblur_train.py; `D.last_path` records which ran:
              * "hip" / "hip-amp": CUDA, fp32 parameters, FUSE_DEBLUR_ADV, x channels-last and 16-byte aligned, and every one of the
                ten activations a whole number of 16-byte lanes (4 fp32 / 8 Half elements).  F.conv2d without bias (MIOpen, plain
                autograd; Half input: on `weight.to(float16)`, autograd's own cast, so the fp32 master weights get fp32 gradients),
                each followed in place by dib_leaky_relu_mask[_f16] through `_LeakyMask`, which keeps the sign mask (one byte per lane)
                instead of the activation and whose backward is one launch (dib_leaky_relu_mask_backward[_f16]).
              * "torch" / "torch-amp": the plain module (under torch.autocast(dtype=float16) for Half input): everything else.
  loss      `adv_bce(logits, real_label)` / `adv_bce_sum([(logits, label), ...])`: mean binary cross-entropy with logits against a
            constant label, all terms added into ONE device scalar by one autograd node (dib_adv_bce_loss per term stores that term's
            gradient; the backward scales it by the incoming gradient) -- `pyramid_l1_loss`'s node.  fp32 logits; the --amp step hands it
            `logits.float()`.  There is no Half loss kernel.  Elsewhere (CPU, tests) `adv_bce_torch`, the same formulas in torch ops.

Summation order of the loss and the depth of its tree: csrc/dib_sliced_sum.h; `adv_loss_depth`."""
import torch
import torch.nn.functional as F
from torch import nn

from .deblur_train import choose_path, lanes, mask_bits_torch, nhwc_grad, sign_mask_torch, sliced_sum_depth, stored_grad_sum

# False: the plain module on the GPU too, for A/B runs (the tests switch it on themselves).  On: 306.04 against 308.49 ms per step at the
# trainer's defaults with --loss 1*L1+1*ADV on an MI355X, 103.64 against 105.47 under --amp; four rounds, the order reversed in every
# other one, the HIP path ahead in each
# (profiles/deblur_adversarial.txt).
FUSE_DEBLUR_ADV = True

SLOPE = 0.2
STRIDES = (1, 2, 1, 2, 1, 4, 1, 4, 1)      # of the nine kernel_size x kernel_size layers; the tenth is 4 x 4, stride 4, padding 0


def _conv_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def final_side(n, kernel_size=5):
    """The side the dense layer sees for an input side n (below 1: the last convolution has no output)."""
    for s in STRIDES:
        n = _conv_out(n, kernel_size, s, (kernel_size - 1) // 2)
    return _conv_out(n, 4, 4, 0)


def min_side(kernel_size=5):
    """The smallest input side the network accepts: 193 at kernel_size 5."""
    n = 1
    while final_side(n, kernel_size) < 1:
        n += 1
    return n


class Discriminator(nn.Module):
    """The reference's models/deblur/discriminator.py: its keys, its shapes, torch's default initialisation."""

    def __init__(self, n_feats=64, kernel_size=5):
        super().__init__()
        self.n_feats, self.kernel_size = n_feats, kernel_size
        f = n_feats
        chans = (3, f // 2, f // 2, f, f, 2 * f, 2 * f, 4 * f, 4 * f, 8 * f)
        layers = [nn.Conv2d(chans[i], chans[i + 1], kernel_size, stride=STRIDES[i], padding=(kernel_size - 1) // 2, bias=False) for i in range(9)]
        layers.append(nn.Conv2d(8 * f, 8 * f, 4, stride=4, padding=0, bias=False))
        self.conv_layers = nn.ModuleList(layers)
        self.act = nn.LeakyReLU(negative_slope=SLOPE, inplace=True)
        self.dense = nn.Conv2d(8 * f, 1, 1, bias=False)
        self.last_path = None

    def check_size(self, x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("Discriminator: needs [B, 3, H, W], got %s" % (tuple(x.shape),))
        if min(final_side(int(x.shape[2]), self.kernel_size), final_side(int(x.shape[3]), self.kernel_size)) < 1:
            raise ValueError("Discriminator: a %d x %d input leaves the last 4 x 4 convolution nothing: the smaller side must be at least %d"
                             % (x.shape[2], x.shape[3], min_side(self.kernel_size)))

    def activation_shapes(self, B, H, W):
        """(B, C, h, w) of the ten activations"""
        out = []
        for conv in self.conv_layers:
            k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
            H, W = _conv_out(H, k, s, p), _conv_out(W, k, s, p)
            out.append((B, conv.out_channels, H, W))
        return out

    def forward(self, x):
        self.check_size(x)
        for layer in self.conv_layers:
            x = self.act(layer(x))
        return self.dense(x)


# ---- LeakyReLU with a sign mask ------------------------------------------------------------------------------------------------------

def leaky_mask_torch(x, slope=SLOPE):
    """dib_leaky_relu_mask[_f16] restated: -> (x > 0 ? x : x * slope with Half multiplied in fp32 and rounded once, the sign mask of the
    result: `sign_mask_torch`, one byte per 4 fp32 / 8 Half elements).  Bit-equal to F.leaky_relu on the CPU; on gfx950 torch's Half
    kernel and dib_leaky_relu_mask_f16 return +0 for -0, the one Half value at which they differ from this."""
    y = torch.where(x > 0, x, (x.float() * slope).to(x.dtype))
    return y, sign_mask_torch(y)


def leaky_grad_torch(grad, mask, slope=SLOPE):
    """dib_leaky_relu_mask_backward[_f16] restated: bit ? grad : grad * slope.  Bit-equal to F.leaky_relu's autograd backward."""
    return torch.where(mask_bits_torch(mask, grad), grad, (grad.float() * slope).to(grad.dtype))


def leaky_mask_device(x, slope=SLOPE, want_mask=True):
    """dib_leaky_relu_mask[_f16] in place on a dense fp32 or Half CUDA tensor -> the mask (None when not asked for)."""
    from .. import _lib
    l = _lib.lib()
    mask = torch.empty(x.numel() // lanes(x.dtype), dtype=torch.uint8, device=x.device) if want_mask else None
    run = l.dib_leaky_relu_mask_f16 if x.dtype == torch.float16 else l.dib_leaky_relu_mask
    _lib.check(run(x.data_ptr(), x.numel(), slope, mask.data_ptr() if want_mask else None, _lib.stream_of(x)))
    return mask


def leaky_grad_device(grad, mask, slope=SLOPE, out=None):
    """dib_leaky_relu_mask_backward[_f16]; `out` may be `grad` itself."""
    from .. import _lib
    l = _lib.lib()
    if out is None:
        out = torch.empty_like(grad)
    run = l.dib_leaky_relu_mask_backward_f16 if grad.dtype == torch.float16 else l.dib_leaky_relu_mask_backward
    _lib.check(run(grad.data_ptr(), mask.data_ptr(), slope, out.data_ptr(), grad.numel(), _lib.stream_of(grad)))
    return out


class _LeakyMask(torch.autograd.Function):
    """x = x > 0 ? x : x * slope in place on a channels-last fp32 or Half CUDA convolution output (dib_leaky_relu_mask[_f16]); what is
    kept for the backward is the sign mask, and the backward is one launch over the gradient (dib_leaky_relu_mask_backward[_f16]).
    Modelled on models/deblur_train.py's `_BiasActTrain`."""

    @staticmethod
    def forward(ctx, x, slope):
        ctx.slope = slope
        mask = leaky_mask_device(x, slope, want_mask=ctx.needs_input_grad[0])
        if mask is not None:
            ctx.save_for_backward(mask)
        ctx.mark_dirty(x)
        return x

    @staticmethod
    def backward(ctx, grad):
        return leaky_grad_device(nhwc_grad(grad), ctx.saved_tensors[0], ctx.slope), None


# ---- the network's two paths ---------------------------------------------------------------------------------------------------------

def _amp(D, x):
    """Half input into fp32 parameters: the mixed-precision step (--amp)."""
    return next(D.parameters()).dtype == torch.float32 and x.dtype == torch.float16


def _hip_ok(D, x):
    p = next(D.parameters())
    lane = lanes(x.dtype)
    return (FUSE_DEBLUR_ADV and p.is_cuda and p.dtype == torch.float32 and x.is_cuda and x.device == p.device
            and x.dtype in (torch.float32, torch.float16) and x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0
            and all(b * c * h * w > 0 and b * c * h * w % lane == 0 for b, c, h, w in D.activation_shapes(int(x.shape[0]), int(x.shape[2]), int(x.shape[3]))))


def _forward_hip(D, x):
    half = x.dtype == torch.float16
    for conv in D.conv_layers:
        # --amp: the cast is autograd's own, so the fp32 master weight gets an fp32 gradient
        y = F.conv2d(x, conv.weight.to(torch.float16) if half else conv.weight, None, conv.stride, conv.padding)
        y = y.contiguous(memory_format=torch.channels_last)                # MIOpen's channels-last kernels give this layout already
        if y.data_ptr() & 15:
            y = y.clone(memory_format=torch.channels_last)
        x = _LeakyMask.apply(y, SLOPE)
    return F.conv2d(x, D.dense.weight.to(torch.float16) if half else D.dense.weight)


def discriminator_forward(D, x):
    """x: [B, 3, H, W] on the 0..255 scale, fp32 or Half (Half into fp32 parameters: the --amp form) -> the logits [B, 1, h, w], one
    per image when the smaller side is 193..., in x's dtype.  `D.last_path`: "hip" / "hip-amp" / "torch" / "torch-amp"."""
    D.check_size(x)
    return choose_path(D, _amp(D, x), _hip_ok(D, x), lambda: _forward_hip(D, x), lambda: D(x))


# ---- the loss ------------------------------------------------------------------------------------------------------------------------

def adv_loss_depth(n):
    """Additions any one term of dib_adv_bce_loss's sum over n logits can pass through."""
    return sliced_sum_depth(n)


def adv_bce_terms_torch(logits, real_label, gscale=1.0):
    """dib_adv_bce_loss restated in torch ops: -> (grad, this term's addend to the loss).  z = -x for label 1, x for label 0;
    term = max(z, 0) + log1p(exp(-|z|)); grad = (label 1: -1, label 0: +1) * gscale / n * sigma(z), sigma without an overflow."""
    z = -logits if real_label else logits
    e = torch.exp(-z.abs())
    n = torch.tensor(float(logits.numel()), dtype=logits.dtype)
    k = (torch.tensor(-gscale if real_label else gscale, dtype=logits.dtype) / n).to(logits.device)
    grad = k * torch.where(z >= 0, 1 / (1 + e), e / (1 + e))
    zero = torch.zeros((), dtype=z.dtype, device=z.device)
    term = torch.where(z > 0, z, zero) + torch.log1p(e)                    # (a NaN z: 0 + NaN)
    return grad, term.sum() / n.to(logits.device)


def _bce_term_torch(x, label, loss):
    grad, term = adv_bce_terms_torch(x, label)
    loss += term
    return grad


def _bce_term_device(x, label, loss):
    return adv_bce_device(x.contiguous(), label, loss).view_as(x)


def adv_bce_torch(logits, real_label):
    """`adv_bce` in torch ops, with the kernel's gradient formula (sigma(0) = 1 / 2, which autograd through max() would not give)."""
    return stored_grad_sum(_bce_term_torch, [logits], [int(real_label)])


def adv_bce_device(logits, real_label, loss, gscale=1.0):
    """dib_adv_bce_loss on contiguous fp32 CUDA logits: adds their mean term into the 1-element `loss`, returns the gradient."""
    from .. import _lib
    l = _lib.lib()
    n = logits.numel()
    grad = torch.empty_like(logits)
    work = torch.empty(max(1, l.dib_adv_bce_loss_workspace_bytes(n) // 4), dtype=torch.float32, device=logits.device)
    _lib.check(l.dib_adv_bce_loss(logits.data_ptr(), n, int(real_label), gscale, grad.data_ptr(), loss.data_ptr(), work.data_ptr(),
                                  _lib.stream_of(logits)))
    return grad


def _bce_hip_ok(logits):
    return FUSE_DEBLUR_ADV and all(x.is_cuda and x.dtype == torch.float32 and x.numel() > 0 for x in logits)


def adv_bce_sum(pairs):
    """sum of mean BCE-with-logits of each (fp32 logits, constant label 0 or 1) pair, one scalar."""
    logits, labels = [p[0] for p in pairs], [int(p[1]) for p in pairs]
    if any(l not in (0, 1) for l in labels):
        raise ValueError("adv_bce: labels are 0 (fake) or 1 (real)")
    return stored_grad_sum(_bce_term_device if _bce_hip_ok(logits) else _bce_term_torch, logits, labels)


def adv_bce(logits, real_label):
    return adv_bce_sum([(logits, real_label)])


def discriminator_loss(net, fake, real):
    """The D update's loss: BCE(D(fake), 0) + BCE(D(real), 1), both into one scalar; `fake` is detached here.  `net`: a callable."""
    return adv_bce_sum([(net(fake.detach()).float(), 0), (net(real).float(), 1)])
