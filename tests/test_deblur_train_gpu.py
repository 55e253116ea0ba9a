"""The DeepDeblur trainer on the GPU: the three kernels of csrc/dib_deblur_train.hip against torch indexing, dib_relu_mask_backward and
float64 sums (error bounds from the depth of each kernel's own summation tree, stated in that file's header), the fused training
path against the plain one with float64 CPU autograd between them, and the driver end to end into the inference stage."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests.test_deblur_train import TINY

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


# ---- (a) dib_deblur_patches -----------------------------------------------------------------------------------------------------

SHAPES = [(3, 20, 28), (3, 17, 40), (3, 12, 12)]


@pytest.mark.parametrize("corner", ["origin", "far"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_patches_bit_equal_to_torch_indexing(dtype, corner):
    from detectinblur_amd.models import deblur_train as DT
    ps = 12
    g = torch.Generator().manual_seed(5)
    # every bit pattern, NaNs and denormals included: the kernel moves values and never converts them
    ibits = torch.int16 if dtype == torch.float16 else torch.int32
    info = torch.iinfo(ibits)
    images = [torch.randint(info.min, info.max, s, generator=g, dtype=torch.int64).to(ibits).view(dtype).cuda() for s in SHAPES]
    for order in ((2, 0, 1), (0, 1, 2)):
        for bits in range(8):
            draws = [DT.PatchDraw(0 if corner == "origin" else s[1] - ps, 0 if corner == "origin" else s[2] - ps,
                                  bool(bits & 1), bool(bits & 2), bool(bits & 4), order) for s in SHAPES]
            got = DT.gather_patches(images, draws, ps)
            want = DT.gather_patches_torch(images, draws, ps)
            assert got.shape == (3, 3, ps, ps) and got.dtype == dtype
            assert torch.equal(_bits(got), _bits(want)), (order, bits)


def test_patches_argument_errors():
    from detectinblur_amd import _lib
    from detectinblur_amd.models import deblur_train as DT
    images = [torch.zeros(3, 12, 12, device="cuda")]
    with pytest.raises(_lib.DibError, match="leaves the"):
        DT.gather_patches(images, [DT.PatchDraw(1, 0, False, False, False, (0, 1, 2))], 12)
    with pytest.raises(_lib.DibError, match="flags"):
        DT.gather_patches(images, [DT.PatchDraw(0, 0, False, False, False, (0, 1, 3))], 12)
    torch.cuda.synchronize()
    assert _lib.lib().dib_device_status(0) == 0


# ---- (b) dib_bias_grad_nhwc ---------------------------------------------------------------------------------------------------------

def _relu_mask_backward(grad, mask):
    from detectinblur_amd import _lib
    out = torch.empty_like(grad)
    _lib.check(_lib.lib().dib_relu_mask_backward(grad.data_ptr(), mask.data_ptr(), out.data_ptr(), grad.numel(), _lib.stream_of(grad)))
    return out


def _check_channel_sums(got, values, depth, what):
    """`got` against the float64 sum of the same fp32 `values` [n_pix, C]: within depth * 2^-24 * sum |values| per channel"""
    want = values.double().sum(0)
    bound = depth * U * values.double().abs().sum(0)
    err = (got.double() - want).abs()
    print(what, "depth", depth, "worst error / bound", float((err / bound.clamp_min(1e-300)).max()))
    assert (err <= bound).all(), what


@pytest.mark.parametrize("n_pix", [1, 5, 255, 256, 257, 4099])
@pytest.mark.parametrize("C", [3, 12, 8, 64])
def test_bias_grad(C, n_pix):
    from detectinblur_amd.models import deblur_train as DT
    g = torch.Generator().manual_seed(1000 * C + n_pix)
    grad = (torch.randn(n_pix, C, generator=g) * torch.rand(n_pix, C, generator=g).mul(6).exp()).cuda()
    depth = DT.bias_grad_depth(n_pix, C)
    # the plain channel sum: nothing is written
    same, bias = DT.bias_grad_device(grad)
    assert same is grad
    _check_channel_sums(bias, grad, depth, "plain C=%d n=%d" % (C, n_pix))
    assert torch.equal(_bits(bias), _bits(DT.bias_grad_device(grad)[1]))                  # two runs: bit-identical
    poisoned = grad.clone()
    poisoned[n_pix // 2, C - 1] = float("nan")
    pb = DT.bias_grad_device(poisoned)[1]
    assert torch.isnan(pb[C - 1]) and torch.equal(_bits(pb[:C - 1]), _bits(bias[:C - 1]))     # one NaN, one channel
    if C % 4:
        return
    y = torch.randn(n_pix, C, generator=g).cuda()
    mask = DT.sign_mask_torch(y)
    want_out = _relu_mask_backward(grad, mask)
    assert torch.equal(_bits(want_out), _bits(DT.bias_grad_torch(grad, mask)[0]))
    out, mbias = DT.bias_grad_device(grad, mask)
    assert out.data_ptr() != grad.data_ptr() and torch.equal(_bits(out), _bits(want_out))
    _check_channel_sums(mbias, want_out, depth, "masked C=%d n=%d" % (C, n_pix))
    aliased = grad.clone()
    out2, mbias2 = DT.bias_grad_device(aliased, mask, out=aliased)                        # in place
    assert out2 is aliased and torch.equal(_bits(aliased), _bits(want_out)) and torch.equal(_bits(mbias2), _bits(mbias))
    # a NaN and an inf that pass the mask reach their own channel's sum only; a masked NaN reaches none
    special = grad.clone()
    ys = y.clone()
    special[0, 0], ys[0, 0] = float("nan"), 1.0
    special[n_pix - 1, C - 1], ys[n_pix - 1, C - 1] = float("inf"), 1.0
    special[n_pix // 2, 1], ys[n_pix // 2, 1] = float("nan"), -1.0
    sout, sbias = DT.bias_grad_device(special, DT.sign_mask_torch(ys))
    assert torch.isnan(sbias[0]) and torch.isinf(sbias[C - 1]) and torch.isfinite(sbias[1:C - 1]).all()
    assert sout[n_pix // 2, 1] == 0


def test_bias_grad_argument_errors():
    from detectinblur_amd import _lib
    l = _lib.lib()
    assert l.dib_bias_grad_workspace_bytes(4099, 64) == 17 * 64 * 4 and l.dib_bias_grad_workspace_bytes(0, 64) == 0
    grad = torch.zeros(8, 3, device="cuda")
    mask = torch.zeros(6, dtype=torch.uint8, device="cuda")
    bias = torch.zeros(3, device="cuda")
    work = torch.zeros(64, device="cuda")
    s = _lib.stream_of(grad)
    assert l.dib_bias_grad_nhwc(grad.data_ptr(), mask.data_ptr(), grad.data_ptr(), 8, 3, bias.data_ptr(), work.data_ptr(), s) == _lib.DIB_EINVAL
    assert b"C % 4" in l.dib_last_error()
    assert l.dib_bias_grad_nhwc(grad.data_ptr(), None, None, 0, 3, bias.data_ptr(), work.data_ptr(), s) == _lib.DIB_EINVAL
    assert l.dib_bias_grad_nhwc(None, None, None, 8, 3, bias.data_ptr(), work.data_ptr(), s) == _lib.DIB_EINVAL
    assert b"null pointer" in l.dib_last_error()


# ---- (c) dib_l1_pyramid_loss ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [6, 3])
@pytest.mark.parametrize("n_pix", [1, 7, 1027])
def test_l1_level(n_pix, stride):
    from detectinblur_amd.models import deblur_train as DT
    g = torch.Generator().manual_seed(10 * n_pix + stride)
    out = (torch.randn(n_pix, 3, generator=g) * 60).cuda()
    target = (torch.randn(n_pix, stride, generator=g) * 60).cuda()
    target[0, 1] = out[0, 1]                                    # a zero difference
    if n_pix > 1:
        out[n_pix // 2, 2], target[n_pix // 2, 2] = -0.0, 0.0   # ... and a negative zero
    d = out.double() - target[:, :3].double()
    loss = torch.zeros(1, device="cuda")
    grad = DT.l1_level_device(out, target, loss)
    k = np.float32(1.0) / np.float32(3 * n_pix)
    assert torch.equal(grad.cpu().double(), (torch.sign(d) * float(k)).cpu())                 # exactly the fp32 constant times the sign
    assert grad[0, 1] == 0
    want = float(d.abs().sum() / (3 * n_pix))
    depth = DT.l1_loss_depth(n_pix)
    bound = (depth + 3) * U * want                              # the subtraction, the tree, the division, the addition onto the scalar
    print("n_pix", n_pix, "stride", stride, "depth", depth, "error", abs(float(loss) - want), "bound", bound)
    assert abs(float(loss) - want) <= bound
    # a second level accumulates into the same scalar; a gradient scale goes into the constant
    out2 = (torch.randn(5, 3, generator=g) * 60).cuda()
    target2 = (torch.randn(5, 3, generator=g) * 60).cuda()
    grad2 = DT.l1_level_device(out2, target2, loss, gscale=0.5)
    d2 = out2.double() - target2.double()
    want2 = float(d2.abs().sum() / 15)
    assert abs(float(loss) - (want + want2)) <= bound + (DT.l1_loss_depth(5) + 3) * U * (want + want2)
    assert torch.equal(grad2.cpu().double(), (torch.sign(d2) * float(np.float32(0.5) / np.float32(15))).cpu())
    # two runs: bit-identical
    again = torch.zeros(1, device="cuda")
    DT.l1_level_device(out, target, again)
    DT.l1_level_device(out2, target2, again, gscale=0.5)
    assert torch.equal(_bits(again), _bits(loss))
    # a NaN difference: a NaN gradient at that element alone, a NaN loss
    out[n_pix - 1, 0] = float("nan")
    nan_loss = torch.zeros(1, device="cuda")
    ng = DT.l1_level_device(out, target, nan_loss)
    assert torch.isnan(ng[n_pix - 1, 0]) and int(torch.isnan(ng).sum()) == 1 and torch.isnan(nan_loss).all()


@pytest.fixture
def fused():
    """the HIP training path switched on, whatever the shipped default is"""
    from detectinblur_amd.models import deblur_train as DT
    saved, DT.FUSE_DEBLUR_TRAIN = DT.FUSE_DEBLUR_TRAIN, True
    yield DT
    DT.FUSE_DEBLUR_TRAIN = saved


def test_l1_pyramid_node_scales_the_stored_gradient(fused):
    DT = fused
    g = torch.Generator().manual_seed(11)
    outs = [(torch.randn(2, 3, s, s, generator=g) * 40).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True) for s in (8, 4)]
    targets = [(torch.randn(2, c, s, s, generator=g) * 40).cuda().contiguous(memory_format=torch.channels_last) for c, s in ((6, 8), (3, 4))]
    loss = DT.pyramid_l1_loss(outs, targets)
    (3.0 * loss).backward()
    plain = [o.detach().clone().requires_grad_(True) for o in outs]
    want = sum(torch.nn.functional.l1_loss(o, t[:, :3]) for o, t in zip(plain, targets))
    (3.0 * want).backward()
    assert abs(float(loss) - float(want)) <= 1e-5 * float(want)
    for o, p in zip(outs, plain):
        assert torch.allclose(o.grad, p.grad, rtol=1e-6, atol=0)


# ---- fused against plain -----------------------------------------------------------------------------------------------------------

def test_fused_training_path_against_plain_with_float64_between():
    """Every parameter gradient of the HIP path and of the plain torch path, on this GPU, against float64 CPU autograd: only the bias
    sums and the loss sum change their order, so the HIP path's worst relative error may be at most 4 x the plain path's."""
    import copy
    from detectinblur_amd.models import deblur
    from detectinblur_amd.models import deblur_train as DT
    torch.manual_seed(6)
    model = deblur.MSResNet(n_scales=2, n_resblocks=2, n_feats=8, kernel_size=5).cuda().to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(7)
    sharp = torch.rand(2, 3, 16, 16, generator=g)
    blurred = ((sharp + torch.roll(sharp, 1, 3) + torch.roll(sharp, 2, 2)) / 3).cuda()
    inputs, targets = DT.patch_levels(blurred, 2), DT.patch_levels(sharp.cuda(), 2)

    def grads(net, ins, tgs):
        for p in net.parameters():
            p.grad = None
        loss = DT.pyramid_l1_loss(DT.msresnet_train_forward(net, ins), tgs)
        loss.backward()
        return float(loss), {k: p.grad.detach().double().cpu() for k, p in net.named_parameters()}

    ref = copy.deepcopy(model).cpu().double()
    loss64, g64 = grads(ref, [l[:, :3].cpu().double().contiguous() for l in inputs], [t[:, :3].cpu().double().contiguous() for t in targets])
    assert ref.last_path == "torch"
    assert DT.FUSE_DEBLUR_TRAIN in (True, False)
    saved = DT.FUSE_DEBLUR_TRAIN
    try:
        DT.FUSE_DEBLUR_TRAIN = True
        loss_hip, g_hip = grads(model, inputs, targets)
        assert model.last_path == "hip"
        DT.FUSE_DEBLUR_TRAIN = False
        loss_plain, g_plain = grads(model, inputs, targets)
        assert model.last_path == "torch"
    finally:
        DT.FUSE_DEBLUR_TRAIN = saved

    def worst(gs):
        return max(float((gs[k] - g64[k]).abs().max() / g64[k].abs().max()) for k in g64)

    e_hip, e_plain = worst(g_hip), worst(g_plain)
    print("worst relative gradient error against float64: hip %.3e, plain %.3e; loss %.6f / %.6f / %.6f" % (e_hip, e_plain, loss_hip, loss_plain, loss64))
    assert set(g_hip) == set(g64) and all(torch.isfinite(v).all() for v in g_hip.values())
    assert abs(loss_hip - loss64) <= 1e-5 * loss64
    assert e_hip <= 4 * e_plain


# ---- end to end ------------------------------------------------------------------------------------------------------------------

def test_driver_trains_on_the_gpu_into_the_inference_stage(tmp_path):
    import re
    from detectinblur_amd import _lib
    from detectinblur_amd import train_deblurrer as TD
    from detectinblur_amd.models import deblur
    from detectinblur_amd.models import deblur_train as DT
    buf = io.StringIO()
    saved = DT.FUSE_DEBLUR_TRAIN
    try:
        DT.FUSE_DEBLUR_TRAIN = True
        with contextlib.redirect_stdout(buf):
            TD.main(["--synthetic", "--synthetic_images", "6", "--synthetic_size", "72", "88", "--device", "cuda", "-j", "0", "-b", "2",
                     "--patch_size", "16", "--print_freq", "1", "--epochs", "1", "--early_stop", "2", "--param_index", "1",
                     "--output_dir", str(tmp_path)] + TINY)
    finally:
        DT.FUSE_DEBLUR_TRAIN = saved
    text = buf.getvalue()
    losses = [float(v) for v in re.findall(r"loss: ([0-9.einfa+-]+)", text)]
    assert len(losses) == 3 and all(np.isfinite(losses)), text[-2000:]
    assert text.count("path: hip") == 3 and "3 steps, 6 images, 0 left out" in text
    with contextlib.redirect_stdout(io.StringIO()):
        d = deblur.Deblurer(str(tmp_path), device="cuda")
    out = d.deblur_(torch.rand(3, 20, 28, device="cuda"))
    assert d.last_path == "hip" and out.shape == (3, 20, 28) and torch.isfinite(out).all()
    torch.cuda.synchronize()
    assert _lib.lib().dib_device_status(0) == 0
