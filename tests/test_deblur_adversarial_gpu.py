"""The trainer's adversarial loss on the GPU: the LeakyReLU kernels of csrc/dib_deblur_adv.hip against torch's own on the same GPU bit
for bit, dib_adv_bce_loss against the float64 definition beside torch's binary_cross_entropy_with_logits, the discriminator's HIP path
against the plain one with float64 CPU autograd between them (fp32 and the --amp form), and the driver end to end.

Measured on an MI355X (printed by the tests; DESIGN.md 4 records them): see each test's docstring."""
import contextlib
import copy
import io
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_deblur_adversarial import SPECIALS, TINY, bce_float64, pattern

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32
TINY32 = float(np.finfo(np.float32).tiny)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same(got, want):
    """bit for bit wherever `want` is not a NaN, a NaN where it is"""
    nan = torch.isnan(want)
    return bool(torch.equal(torch.isnan(got), nan) and torch.equal(_bits(got)[~nan], _bits(want)[~nan]))


@pytest.fixture
def fused():
    """the HIP path switched on, whatever the shipped default is"""
    from detectinblur_amd.models import deblur_adversarial as DA
    saved, DA.FUSE_DEBLUR_ADV = DA.FUSE_DEBLUR_ADV, True
    yield DA
    DA.FUSE_DEBLUR_ADV = saved


# ---- LeakyReLU -------------------------------------------------------------------------------------------------------------------

def _any_bits(n, dtype, seed):
    """n elements of random bit patterns (NaNs, infinities and denormals among them), the named special values in front"""
    ibits = torch.int16 if dtype == torch.float16 else torch.int32
    info = torch.iinfo(ibits)
    x = torch.randint(info.min, info.max, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int64).to(ibits).view(dtype)
    denormal = 6e-8 if dtype == torch.float16 else 1e-41
    special = torch.tensor([0.0, -0.0, float("nan"), float("inf"), float("-inf"), denormal, -denormal, 65504.0, -65504.0]).to(dtype)
    k = min(n, special.numel())
    x[:k] = special[:k]
    return x.cuda()


@pytest.mark.parametrize("n_vec", [1, 255, 256, 257, 4099])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_leaky_relu_kernels_equal_torchs_bit_for_bit(dtype, n_vec):
    from detectinblur_amd import _lib
    from detectinblur_amd.models import deblur_adversarial as DA
    from detectinblur_amd.models.deblur_train import sign_mask_torch
    lane = 8 if dtype == torch.float16 else 4
    x = _any_bits(n_vec * lane, dtype, 100 * n_vec + lane)
    want = F.leaky_relu_(x.clone(), 0.2)
    got = x.clone()
    mask = DA.leaky_mask_device(got, 0.2)
    assert _same(got, want)
    assert mask.dtype == torch.uint8 and mask.numel() == n_vec and torch.equal(mask, sign_mask_torch(got))
    # the restatement in torch ops: equal too, up to the sign of a zero (torch's Half kernel on this GPU returns +0 for -0)
    restated = DA.leaky_mask_torch(x)[0]
    assert _same(restated + 0, got + 0) and torch.equal(restated == 0, got == 0)
    bare = x.clone()
    assert DA.leaky_mask_device(bare, 0.2, want_mask=False) is None and torch.equal(_bits(bare), _bits(got))      # a null mask
    # the backward against torch's autograd on the same GPU
    g = _any_bits(n_vec * lane, dtype, 7 + n_vec)
    leaf = x.clone().requires_grad_(True)
    F.leaky_relu(leaf, 0.2).backward(g)
    out = DA.leaky_grad_device(g, mask, 0.2)
    assert out.data_ptr() != g.data_ptr() and _same(out, leaf.grad)
    aliased = g.clone()
    assert DA.leaky_grad_device(aliased, mask, 0.2, out=aliased) is aliased and torch.equal(_bits(aliased), _bits(out))      # out == g
    torch.cuda.synchronize()
    assert _lib.lib().dib_device_status(0) == 0


def test_leaky_relu_f16_equals_torchs_at_every_half_value():
    """all 65536 Half bit patterns, forward and (as the gradient, against every pattern as the input, reversed) backward: what
    csrc/dib_deblur_adv.hip's `leak` rests on -- torch's Half kernel returns +0 for -0, and so does dib_leaky_relu_mask_f16"""
    from detectinblur_amd.models import deblur_adversarial as DA
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.float16).cuda()
    got = x.clone()
    mask = DA.leaky_mask_device(got, 0.2)
    assert _same(got, F.leaky_relu_(x.clone(), 0.2))
    for g in (x.flip(0).contiguous(), x.roll(12345).contiguous(), torch.full_like(x, -0.0)):
        leaf = x.clone().requires_grad_(True)
        F.leaky_relu(leaf, 0.2).backward(g)
        assert _same(DA.leaky_grad_device(g, mask, 0.2), leaf.grad)


def test_leaky_relu_refusals():
    from detectinblur_amd import _lib
    l = _lib.lib()
    x = torch.zeros(64, device="cuda")
    h = torch.zeros(64, device="cuda", dtype=torch.float16)
    mask = torch.zeros(16, dtype=torch.uint8, device="cuda")
    s = _lib.stream_of(x)
    E = _lib.DIB_EINVAL
    for slope in (0.0, -0.2, float("nan"), float("inf")):
        assert l.dib_leaky_relu_mask(x.data_ptr(), 64, slope, mask.data_ptr(), s) == E and b"slope" in l.dib_last_error()
        assert l.dib_leaky_relu_mask_f16(h.data_ptr(), 64, slope, mask.data_ptr(), s) == E and b"slope" in l.dib_last_error()
        assert l.dib_leaky_relu_mask_backward(x.data_ptr(), mask.data_ptr(), slope, x.data_ptr(), 64, s) == E and b"slope" in l.dib_last_error()
        assert l.dib_leaky_relu_mask_backward_f16(h.data_ptr(), mask.data_ptr(), slope, h.data_ptr(), 64, s) == E and b"slope" in l.dib_last_error()
    assert l.dib_leaky_relu_mask(x.data_ptr(), 62, 0.2, None, s) == E and b"multiple of 4" in l.dib_last_error()
    assert l.dib_leaky_relu_mask(x.data_ptr(), -4, 0.2, None, s) == E and b"multiple of 4" in l.dib_last_error()
    assert l.dib_leaky_relu_mask_f16(h.data_ptr(), 60, 0.2, None, s) == E and b"multiple of 8" in l.dib_last_error()
    assert l.dib_leaky_relu_mask_backward(x.data_ptr(), mask.data_ptr(), 0.2, x.data_ptr(), 63, s) == E and b"multiple of 4" in l.dib_last_error()
    assert l.dib_leaky_relu_mask_backward_f16(h.data_ptr(), mask.data_ptr(), 0.2, h.data_ptr(), 4, s) == E and b"multiple of 8" in l.dib_last_error()
    assert l.dib_leaky_relu_mask(None, 64, 0.2, mask.data_ptr(), s) == E and b"null pointer" in l.dib_last_error()
    assert l.dib_leaky_relu_mask_f16(None, 64, 0.2, None, s) == E and b"null pointer" in l.dib_last_error()
    assert l.dib_leaky_relu_mask_backward(x.data_ptr(), None, 0.2, x.data_ptr(), 64, s) == E and b"null pointer" in l.dib_last_error()
    assert l.dib_leaky_relu_mask_backward_f16(h.data_ptr(), mask.data_ptr(), 0.2, None, 64, s) == E and b"null pointer" in l.dib_last_error()
    assert l.dib_leaky_relu_mask(x.data_ptr() + 4, 32, 0.2, None, s) == E and b"16-byte aligned" in l.dib_last_error()
    assert l.dib_leaky_relu_mask_f16(h.data_ptr() + 2, 32, 0.2, None, s) == E and b"16-byte aligned" in l.dib_last_error()
    assert l.dib_leaky_relu_mask_backward(x.data_ptr(), mask.data_ptr(), 0.2, x.data_ptr() + 8, 32, s) == E and b"16-byte aligned" in l.dib_last_error()
    assert l.dib_leaky_relu_mask_backward_f16(h.data_ptr() + 8, mask.data_ptr(), 0.2, h.data_ptr(), 32, s) == E and b"16-byte aligned" in l.dib_last_error()
    # nothing to do is not an error, whatever the pointers
    assert l.dib_leaky_relu_mask(None, 0, 0.2, None, s) == 0 and l.dib_leaky_relu_mask_backward_f16(None, None, 0.2, None, 0, s) == 0
    torch.cuda.synchronize()
    assert not x.any() and not h.any() and _lib.lib().dib_device_status(0) == 0


# ---- dib_adv_bce_loss --------------------------------------------------------------------------------------------------------------

SIZES = [1, 2, 16, 257, 2049, 2048 * 1024 + 5]


def _logits(n):
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 8
    k = min(n, len(SPECIALS))
    x[n - k:] = torch.tensor(SPECIALS[:k])              # (at the end: the last slice's tail)
    return x.cuda()


def _relative(grad, want):
    """worst element-wise relative error against float64, the denominator floored at fp32's smallest normal"""
    return float(((grad.double() - want).abs() / want.abs().clamp_min(TINY32)).max())


@pytest.fixture(scope="module")
def torchs_worst():
    """label -> the worst relative gradient error of F.binary_cross_entropy_with_logits in fp32 on this GPU over the test's sizes"""
    worst = {}
    for label in (0, 1):
        errs = []
        for n in SIZES:
            x = _logits(n).requires_grad_(True)
            F.binary_cross_entropy_with_logits(x, torch.full_like(x, float(label))).backward()
            errs.append(_relative(x.grad, bce_float64(x.detach(), label)[0] / n))
        worst[label] = max(errs)
    return worst


@pytest.mark.parametrize("label", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_adv_bce_loss_against_float64_beside_torch(n, label, torchs_worst):
    """The gradient: worst relative error at most 4 x the worst of torch's own binary_cross_entropy_with_logits (over these sizes, same
    label) -- whose sigmoid(x) - 1 cancels for label 1, so that bound alone says little there -- AND at most 8 x 2^-24 by the kernel's
    own arithmetic: expf within one unit of 2^-23, then 1 + e, the division, k = gscale / n and the product, each rounding once
    (2^-23 + 4 x 2^-24 = 6 x 2^-24, to first order).  The loss: at most 4 x torch's own error plus adv_loss_depth(n) x 2^-24 x mean for
    the sum's order."""
    from detectinblur_amd.models import deblur_adversarial as DA
    x = _logits(n)
    g64, t64 = bce_float64(x, label)
    want = float(t64.sum() / n)
    loss = torch.zeros(1, device="cuda")
    grad = DA.adv_bce_device(x, label, loss)
    leaf = x.clone().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(leaf, torch.full_like(x, float(label)))
    e_kernel, e_torch = _relative(grad, g64 / n), torchs_worst[label]
    l_kernel, l_torch = abs(float(loss) - want), abs(float(ref.detach()) - want)
    depth = DA.adv_loss_depth(n)
    print("n", n, "label", label, "gradient: kernel %.3e, torch's worst %.3e; loss: kernel %.3e, torch %.3e, depth %d, value %.6f"
          % (e_kernel, e_torch, l_kernel, l_torch, depth, want))
    assert e_kernel <= 4 * e_torch and e_kernel <= 8 * U
    assert l_kernel <= 4 * l_torch + depth * U * want
    # gscale lands in the constant; a second call accumulates into the same scalar
    x2 = _logits(16)
    grad2 = DA.adv_bce_device(x2, 1 - label, loss, gscale=0.5)
    assert _relative(grad2, 0.5 * bce_float64(x2, 1 - label)[0] / 16) <= 8 * U
    want2 = float(bce_float64(x2, 1 - label)[1].sum() / 16)
    assert abs(float(loss) - (want + want2)) <= l_kernel + (DA.adv_loss_depth(16) + 2) * U * (want + want2) + 4 * U * want2
    # two runs: bit-identical
    again = torch.zeros(1, device="cuda")
    grad_again = DA.adv_bce_device(x, label, again)
    DA.adv_bce_device(x2, 1 - label, again, gscale=0.5)
    assert torch.equal(_bits(again), _bits(loss)) and torch.equal(_bits(grad_again), _bits(grad))
    # a NaN logit: a NaN at its own gradient element, a NaN loss, nothing else
    x[n // 2] = float("nan")
    nan_loss = torch.zeros(1, device="cuda")
    ng = DA.adv_bce_device(x, label, nan_loss)
    assert torch.isnan(ng[n // 2]) and int(torch.isnan(ng).sum()) == 1 and torch.isnan(nan_loss).all()
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[n // 2] = False
    assert torch.equal(_bits(ng[keep]), _bits(grad[keep]))


@pytest.mark.parametrize("label", [0, 1])
@pytest.mark.parametrize("n", [1, 257, 2049, 4099, 2048 * 1024, 2048 * 1024 + 5],
                         ids=["1", "257", "2049-two-uneven-slices", "4099", "S1024-exactly", "capped-five-longer-slices"])
def test_adv_bce_stated_order(n, label):
    """The sum's order bit for bit: csrc/dib_sliced_sum.h's, as tests/test_deblur_train.py restates it in numpy float32 (`_walk`).  expf
    and log1pf cannot be restated bit for bit, so the logits are chosen where the term does not depend on them: |x| >= 110 on the side
    of the label at which z = |x|.  exp(-110) = 1.7e-48 lies below half the smallest fp32 denormal (7e-46), so e = expf(-|z|) is exactly
    0 with or without denormal flushing, log1pf(0) is 0, the term is z itself and sigma is exactly 1: the loss is `_walk` over z, one
    division by float32(n) and one addition onto a scalar that is not zero, and every gradient element is -+(float32(gscale) /
    float32(n))."""
    from detectinblur_amd.models import deblur_adversarial as DA
    from tests.test_deblur_train import _F32, _real_draw, _walk, slice_begins
    gscale, start = 0.75, 3.25
    z = np.float32(110) + np.abs(_real_draw(np.random.RandomState(7 * n + label), n))
    assert z.dtype == np.float32 and (z >= 110).all() and np.isfinite(z).all()
    S = max(1, min(1024, -(-n // 2048)))
    assert DA.adv_loss_depth(n) == -(-int(np.diff(slice_begins(n, S)).max()) // 256) + 8 + S - 1
    want = np.float32(start) + _walk(n, S, 256, _F32(z)) / np.float32(n)
    assert np.isfinite(want) and want.dtype == np.float32
    k = np.float32(gscale) / np.float32(n)
    x = torch.from_numpy(-z if label else z).cuda()
    loss = torch.full((1,), start, device="cuda")
    grad = DA.adv_bce_device(x, label, loss, gscale=gscale)
    print("n", n, "label", label, "S", S, "loss %.9g, stated %.9g" % (float(loss), float(want)))
    assert np.array_equal(loss.cpu().numpy().view(np.int32), np.array([want]).view(np.int32)), (float(loss), float(want))
    assert np.array_equal(grad.cpu().numpy().view(np.int32), np.full(n, -k if label else k, dtype=np.float32).view(np.int32))


def test_adv_bce_refusals_and_the_node(fused):
    from detectinblur_amd import _lib
    DA = fused
    l = _lib.lib()
    assert l.dib_adv_bce_loss_workspace_bytes(0) == 0 and l.dib_adv_bce_loss_workspace_bytes(2049) == 8
    assert l.dib_adv_bce_loss_workspace_bytes(2048 * 1024 + 5) == 4096
    x = torch.zeros(8, device="cuda")
    s = _lib.stream_of(x)
    p = x.data_ptr()
    assert l.dib_adv_bce_loss(p, 0, 1, 1.0, p, p, p, s) == _lib.DIB_EINVAL and b"0 < n" in l.dib_last_error()
    assert l.dib_adv_bce_loss(p, 8, 2, 1.0, p, p, p, s) == _lib.DIB_EINVAL and b"real_label" in l.dib_last_error()
    assert l.dib_adv_bce_loss(p, 8, 1, 1.0, None, p, p, s) == _lib.DIB_EINVAL and b"null pointer" in l.dib_last_error()
    assert l.dib_adv_bce_loss(p + 2, 8, 1, 1.0, p, p, p, s) == _lib.DIB_EINVAL and b"4-byte aligned" in l.dib_last_error()
    # the node: both terms into one scalar, the stored gradients scaled by the incoming one
    a, b = _logits(257).reshape(257, 1, 1, 1).requires_grad_(True), _logits(16).requires_grad_(True)
    loss = DA.adv_bce_sum([(a, 0), (b, 1)])
    (3.0 * loss).backward()
    a2, b2 = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(a2, torch.zeros_like(a2)) + F.binary_cross_entropy_with_logits(b2, torch.ones_like(b2))
    (3.0 * ref).backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-6 * float(ref.detach())
    assert torch.allclose(a.grad, a2.grad, rtol=1e-5, atol=3.0 * 4 * U / 257) and torch.allclose(b.grad, b2.grad, rtol=1e-5, atol=3.0 * 4 * U / 16)
    torch.cuda.synchronize()
    assert l.dib_device_status(0) == 0


# ---- the discriminator: HIP path against plain path, float64 between ---------------------------------------------------------------

LOSS_SCALE = 2.0 ** 16      # a power of two: exact in every format, and taken out again in float64


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "amp"])
def test_discriminator_hip_path_against_plain_with_float64_between(fused, dtype):
    """The logits, every parameter gradient and the input gradient of BCE(D(x), 1) on the HIP path and on the plain path (for Half input:
    autocast), on this GPU, against float64 CPU autograd of the same module on the same input values.  The backward runs on the loss
    times 2^16, as the --amp step runs it on a scaled loss (unscaled, the float64 input gradient, 2.3e-7 at most, lies below Half's
    smallest normal and the comparison would measure underflow), and the scale is divided out in float64.  TENSOR BY TENSOR, with
    e[k] = max |g[k] - g64[k]| / max |g64[k]|:
      * the HIP path's error is at most 4 x the plain path's for that tensor (the LeakyReLU kernels are torch's bit for bit, so only
        the loss's order, the place of the casts and MIOpen's own run-to-run order differ);
      * the two paths agree with each other directly, max |g_hip[k] - g_plain[k]| / max |g64[k]| <= 4 x the plain path's error: what a
        dropped layer or a wrong mask breaks (a backward of zeros is 1.0 off).
    The logits agree with float64 to 1e-5 of max |logit| in fp32; with Half input to 4 x the autocast path's own logit error on top."""
    DA = fused
    torch.manual_seed(9)
    D = DA.Discriminator(n_feats=8).cuda().to(memory_format=torch.channels_last)
    x = pattern(2, 196, 196).cuda().to(dtype).contiguous(memory_format=torch.channels_last)

    def grads(net, inp):
        for p in net.parameters():
            p.grad = None
        inp = inp.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
        logits = DA.discriminator_forward(net, inp)
        loss = DA.adv_bce(logits if logits.dtype == torch.float64 else logits.float(), 1)
        (loss * LOSS_SCALE).backward()
        gs = {k: p.grad.detach().double().cpu() / LOSS_SCALE for k, p in net.named_parameters()}
        gs["input"] = inp.grad.detach().double().cpu() / LOSS_SCALE
        return logits.detach().double().cpu(), float(loss.detach()), gs

    ref = copy.deepcopy(D).cpu().double()
    logits64, loss64, g64 = grads(ref, x.cpu().double().contiguous())
    assert ref.last_path == "torch"
    hip, plain = ("hip", "torch") if dtype == torch.float32 else ("hip-amp", "torch-amp")
    logits_hip, loss_hip, g_hip = grads(D, x)
    assert D.last_path == hip
    assert all(p.grad.dtype == torch.float32 for p in D.parameters())
    DA.FUSE_DEBLUR_ADV = False
    logits_plain, loss_plain, g_plain = grads(D, x)
    assert D.last_path == plain
    assert set(g_hip) == set(g64) and len(g_hip) == 12 and all(torch.isfinite(v).all() for v in g_hip.values())

    def off(a, b, k):
        return float((a[k] - b[k]).abs().max() / g64[k].abs().max())

    failures = []
    for k in g64:
        e_hip, e_plain, between = off(g_hip, g64, k), off(g_plain, g64, k), off(g_hip, g_plain, k)
        print("%s %-22s %s %.3e  %s %.3e  between the two %.3e  (max |g64| %.3e)" % (dtype, k, hip, e_hip, plain, e_plain, between, float(g64[k].abs().max())))
        if not (e_plain > 0 and e_hip <= 4 * e_plain and between <= 4 * e_plain):
            failures.append(k)
    top = float(logits64.abs().max())
    l_hip, l_plain = float((logits_hip - logits64).abs().max()) / top, float((logits_plain - logits64).abs().max()) / top
    print("%s logits %s: %s %.3e, %s %.3e of max |logit|; loss %.7f / %.7f / %.7f"
          % (dtype, logits64.flatten().tolist(), hip, l_hip, plain, l_plain, loss_hip, loss_plain, loss64))
    assert not failures, failures
    assert logits_hip.shape == logits64.shape == (2, 1, 1, 1)
    assert l_hip <= 1e-5 + (0 if dtype == torch.float32 else 4 * l_plain)
    assert abs(loss_hip - loss64) <= 1e-5 * loss64 + (0 if dtype == torch.float32 else 4 * abs(loss_plain - loss64))


# ---- end to end ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
def test_driver_trains_with_adv_on_the_gpu_into_the_inference_stage(fused, tmp_path, amp):
    from detectinblur_amd import _lib
    from detectinblur_amd import train_deblurrer as TD
    from detectinblur_amd.models import deblur
    from detectinblur_amd.models import deblur_train as DT
    buf = io.StringIO()
    saved = DT.FUSE_DEBLUR_TRAIN, DT.FUSE_DEBLUR_TRAIN_AMP
    try:
        DT.FUSE_DEBLUR_TRAIN = DT.FUSE_DEBLUR_TRAIN_AMP = True
        with contextlib.redirect_stdout(buf):
            TD.main(["--synthetic", "--synthetic_images", "6", "--synthetic_size", "200", "216", "--device", "cuda", "-j", "0", "-b", "2",
                     "--patch_size", "196", "--print_freq", "1", "--epochs", "1", "--early_stop", "2", "--param_index", "1",
                     "--output_dir", str(tmp_path), "--loss", "1*L1+1*ADV"] + TINY + (["--amp"] if amp else []))
    finally:
        DT.FUSE_DEBLUR_TRAIN, DT.FUSE_DEBLUR_TRAIN_AMP = saved
    text = buf.getvalue()
    path = "hip-amp" if amp else "hip"
    rows = re.findall(r"loss: (\S+)  lr: \S+  path: %s  adv: (\S+)  d: (\S+)  d_path: %s(?:  scale: (\S+))?\n" % (path, path), text)
    assert len(rows) == 3 and all(np.isfinite(float(v)) for row in rows for v in row[:3]), text[-2000:]
    assert all(bool(row[3]) == amp for row in rows) and "3 steps, 6 images, 0 left out" in text
    state = torch.load(tmp_path / "models" / "model-1.pt", map_location="cpu", weights_only=True)
    assert set(state) == {"G", "D"} and all(v.dtype == torch.float32 for part in state.values() for v in part.values())
    with contextlib.redirect_stdout(io.StringIO()):
        d = deblur.Deblurer(str(tmp_path), device="cuda")
    out = d.deblur_(torch.rand(3, 20, 28, device="cuda"))
    assert out.shape == (3, 20, 28) and torch.isfinite(out).all()
    torch.cuda.synchronize()
    assert _lib.lib().dib_device_status(0) == 0
