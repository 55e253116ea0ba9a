"""The trainer's mixed-precision step (--amp) on the GPU: dib_bias_act_mask_f16_nhwc against dib_bias_act_f16_nhwc's stored bits,
dib_bias_grad_f16_nhwc against float64 sums (the bound of the fp32 form: depth of the kernel's own summation tree x 2^-24 x sum |g|,
the Half inputs being exact in fp32) and against the select restated in torch, the Half training path against its restatement bit for
bit and against float64 CPU autograd beside the autocast path, and the driver end to end."""
import contextlib
import copy
import io
import re

import numpy as np
import pytest
import torch

from tests.test_deblur_train import TINY

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@pytest.fixture
def fused():
    """the Half HIP training path switched on, whatever the shipped defaults are"""
    from detectinblur_amd.models import deblur_train as DT
    saved = DT.FUSE_DEBLUR_TRAIN, DT.FUSE_DEBLUR_TRAIN_AMP
    DT.FUSE_DEBLUR_TRAIN = DT.FUSE_DEBLUR_TRAIN_AMP = True
    yield DT
    DT.FUSE_DEBLUR_TRAIN, DT.FUSE_DEBLUR_TRAIN_AMP = saved


# ---- dib_bias_act_mask_f16_nhwc ------------------------------------------------------------------------------------------------------

def _epilogue_inputs(n_pix, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n_pix, C, generator=g) * 4).half()
    bias = torch.randn(C, generator=g)                     # fp32 values that are no Half values
    res = (torch.randn(n_pix, C, generator=g) * 4).half()
    # the first pixel's eight channels: +0, -0, NaN, +inf, -inf, a Half denormal, and two sums beyond 65504
    x[0, :8] = torch.tensor([0.0, -0.0, float("nan"), float("inf"), float("-inf"), 6e-8, 65504.0, -65504.0]).half()
    bias[:8] = torch.tensor([0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 40.0, -40.0])
    res[0, :8] = torch.tensor([0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 60000.0, -60000.0]).half()
    return x.cuda(), bias.cuda(), res.cuda()


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("n_pix", [1, 5, 257])
@pytest.mark.parametrize("C", [8, 64])
def test_bias_act_mask_f16(C, n_pix, with_res):
    from detectinblur_amd import _lib
    from detectinblur_amd.models import deblur_train as DT
    l = _lib.lib()
    x, bias, res = _epilogue_inputs(n_pix, C, 100 * C + n_pix)
    rp = res.data_ptr() if with_res else None
    want = x.clone()
    _lib.check(l.dib_bias_act_f16_nhwc(want.data_ptr(), bias.data_ptr(), rp, want.numel(), C, 1, _lib.stream_of(x)))
    got = x.clone()
    mask = torch.full((got.numel() // 8,), 0xAA, dtype=torch.uint8, device="cuda")
    _lib.check(l.dib_bias_act_mask_f16_nhwc(got.data_ptr(), bias.data_ptr(), rp, got.numel(), C, mask.data_ptr(), _lib.stream_of(x)))
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(mask, DT.sign_mask_torch(got))
    # the restatement in torch ops on the same values: the arithmetic the network's restatement relies on
    t = (x.float() + bias).half()
    if with_res:
        t = (t.float() + res.float()).half()
    t = torch.relu(t)
    assert torch.equal(_bits(got), _bits(t))
    first = got[0, :8].float().cpu()
    assert torch.isnan(first[2]) and first[3] == float("inf") and first[4] == 0 and first[7] == 0
    assert first[6] == float("inf")                                        # 65504 + 40 lies above 65520, the last value that rounds back
    assert int(mask[0]) == (1 << 3) | (1 << 5) | (1 << 6)                   # +inf, the denormal, the large value; no bit for the NaN


def test_bias_act_mask_f16_argument_errors():
    from detectinblur_amd import _lib
    l = _lib.lib()
    x = torch.zeros(5 * 24 + 8, dtype=torch.float16, device="cuda")
    bias = torch.zeros(24, device="cuda")
    mask = torch.zeros(32, dtype=torch.uint8, device="cuda")
    s = _lib.stream_of(x)
    before = x.clone()
    assert l.dib_bias_act_mask_f16_nhwc(x.data_ptr(), bias.data_ptr(), None, 5 * 12, 12, mask.data_ptr(), s) == _lib.DIB_EINVAL
    assert b"C % 8" in l.dib_last_error()
    assert l.dib_bias_act_mask_f16_nhwc(x.data_ptr() + 2, bias.data_ptr(), None, 5 * 24, 24, mask.data_ptr(), s) == _lib.DIB_EINVAL
    assert b"16-byte aligned" in l.dib_last_error()
    assert l.dib_bias_act_mask_f16_nhwc(x.data_ptr(), bias.data_ptr(), x.data_ptr() + 8, 5 * 24, 24, mask.data_ptr(), s) == _lib.DIB_EINVAL
    assert l.dib_bias_act_mask_f16_nhwc(x.data_ptr(), bias.data_ptr(), None, 5 * 24, 24, None, s) == _lib.DIB_EINVAL
    assert b"null pointer" in l.dib_last_error()
    assert l.dib_bias_act_mask_f16_nhwc(None, bias.data_ptr(), None, 5 * 24, 24, mask.data_ptr(), s) == _lib.DIB_EINVAL
    assert l.dib_bias_act_mask_f16_nhwc(x.data_ptr(), bias.data_ptr(), None, 0, 24, mask.data_ptr(), s) == 0      # empty: nothing to do
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), _bits(before)) and l.dib_device_status(0) == 0


# ---- dib_bias_grad_f16_nhwc -----------------------------------------------------------------------------------------------------------

def _check_channel_sums(got, values, depth, what):
    """`got` against the float64 sum of the same Half `values` [n_pix, C]: within depth * 2^-24 * sum |values| per channel"""
    want = values.double().sum(0)
    bound = depth * U * values.double().abs().sum(0)
    err = (got.double() - want).abs()
    print(what, "depth", depth, "worst error / bound", float((err / bound.clamp_min(1e-300)).max()))
    assert (err <= bound).all(), what


@pytest.mark.parametrize("n_pix,C", [(n, C) for C in (3, 12, 8, 64) for n in (1, 5, 255, 256, 257, 4099)] + [(5, 2056)])
def test_bias_grad_f16(C, n_pix):
    from detectinblur_amd.models import deblur_train as DT
    g = torch.Generator().manual_seed(1000 * C + n_pix)
    # drawn as the fp32 test draws (magnitudes up to e^6 = 403 x a normal deviate: all finite in Half), rounded to Half
    grad = (torch.randn(n_pix, C, generator=g) * torch.rand(n_pix, C, generator=g).mul(6).exp()).half().cuda()
    assert torch.isfinite(grad).all() and grad.data_ptr() % 16 == 0
    V = DT.bias_grad_lanes(C, torch.float16)
    depth = DT.bias_grad_depth(n_pix, C, V=V)
    same, bias = DT.bias_grad_device(grad)
    assert same is grad and bias.dtype == torch.float32
    _check_channel_sums(bias, grad, depth, "plain C=%d n=%d" % (C, n_pix))
    assert torch.equal(_bits(bias), _bits(DT.bias_grad_device(grad)[1]))                  # two runs: bit-identical
    poisoned = grad.clone()
    poisoned[n_pix // 2, C - 1] = float("nan")
    pb = DT.bias_grad_device(poisoned)[1]
    assert torch.isnan(pb[C - 1]) and torch.equal(_bits(pb[:C - 1]), _bits(bias[:C - 1]))     # one NaN, one channel
    if C % 8:
        return
    y = torch.randn(n_pix, C, generator=g).half().cuda()
    mask = DT.sign_mask_torch(y)
    want_out = torch.where(y > 0, grad, torch.zeros((), dtype=torch.float16, device="cuda"))  # +0 where the bit is clear
    assert torch.equal(_bits(want_out), _bits(DT.bias_grad_torch(grad, mask)[0]))
    out, mbias = DT.bias_grad_device(grad, mask)
    assert out.data_ptr() != grad.data_ptr() and out.dtype == torch.float16 and torch.equal(_bits(out), _bits(want_out))
    _check_channel_sums(mbias, want_out, depth, "masked C=%d n=%d" % (C, n_pix))
    assert torch.equal(_bits(mbias), _bits(DT.bias_grad_device(grad, mask)[1]))
    aliased = grad.clone()
    out2, mbias2 = DT.bias_grad_device(aliased, mask, out=aliased)                        # in place
    assert out2 is aliased and torch.equal(_bits(aliased), _bits(want_out)) and torch.equal(_bits(mbias2), _bits(mbias))
    # a NaN and an inf that pass the mask reach their own channel's sum only; a masked NaN reaches none; -0 passes as -0
    special, ys = grad.clone(), y.clone()
    special[0, 0], ys[0, 0] = float("nan"), 1.0
    special[n_pix - 1, C - 1], ys[n_pix - 1, C - 1] = float("inf"), 1.0
    special[n_pix // 2, 1], ys[n_pix // 2, 1] = float("nan"), -1.0
    special[n_pix // 2, 2], ys[n_pix // 2, 2] = -0.0, 1.0
    sout, sbias = DT.bias_grad_device(special, DT.sign_mask_torch(ys))
    assert torch.isnan(sbias[0]) and torch.isinf(sbias[C - 1]) and torch.isfinite(sbias[1:C - 1]).all()
    assert int(_bits(sout)[n_pix // 2, 1]) == 0 and int(_bits(sout)[n_pix // 2, 2]) == -32768


def test_bias_grad_f16_takes_one_channel_per_lane_off_sixteen_bytes():
    """C % 8 == 0 on a gradient that is only 2-byte aligned: the V = 1 order, and its bound"""
    from detectinblur_amd import _lib
    from detectinblur_amd.models import deblur_train as DT
    l = _lib.lib()
    n_pix, C = 257, 8
    g = torch.Generator().manual_seed(9)
    buf = (torch.randn(n_pix * C + 8, generator=g) * 50).half().cuda()
    grad = buf[1:1 + n_pix * C].view(n_pix, C)
    assert grad.data_ptr() % 16 == 2
    bias = torch.empty(C, device="cuda")
    work = torch.empty(l.dib_bias_grad_f16_workspace_bytes(n_pix, C) // 4, device="cuda")
    _lib.check(l.dib_bias_grad_f16_nhwc(grad.data_ptr(), None, None, n_pix, C, bias.data_ptr(), work.data_ptr(), _lib.stream_of(grad)))
    _check_channel_sums(bias, grad, DT.bias_grad_depth(n_pix, C, V=1), "misaligned C=8")


def test_bias_grad_f16_argument_errors():
    from detectinblur_amd import _lib
    l = _lib.lib()
    # sized for the one-channel-per-lane form, which has the shorter slices: 4 rows x 16 pixels at C = 64 -> ceil(4099 / 64) = 65 slices
    assert l.dib_bias_grad_f16_workspace_bytes(4099, 64) == 65 * 64 * 4 and l.dib_bias_grad_f16_workspace_bytes(0, 64) == 0
    assert l.dib_bias_grad_f16_workspace_bytes(16 * 256 * 256, 64) == 1024 * 64 * 4
    grad = torch.zeros(8 * 12 + 8, dtype=torch.float16, device="cuda")
    mask = torch.zeros(16, dtype=torch.uint8, device="cuda")
    bias = torch.zeros(16, device="cuda")
    work = torch.zeros(256, device="cuda")
    s = _lib.stream_of(grad)
    run = l.dib_bias_grad_f16_nhwc
    assert run(grad.data_ptr(), mask.data_ptr(), grad.data_ptr(), 8, 12, bias.data_ptr(), work.data_ptr(), s) == _lib.DIB_EINVAL
    assert b"C % 8" in l.dib_last_error()
    assert run(grad.data_ptr(), mask.data_ptr(), None, 8, 8, bias.data_ptr(), work.data_ptr(), s) == _lib.DIB_EINVAL
    assert b"without grad_out_dev" in l.dib_last_error()
    assert run(grad.data_ptr() + 2, mask.data_ptr(), grad.data_ptr() + 2, 8, 8, bias.data_ptr(), work.data_ptr(), s) == _lib.DIB_EINVAL
    assert b"16-byte aligned" in l.dib_last_error()
    assert run(grad.data_ptr() + 1, None, None, 8, 8, bias.data_ptr(), work.data_ptr(), s) == _lib.DIB_EINVAL
    assert run(grad.data_ptr(), None, None, 0, 3, bias.data_ptr(), work.data_ptr(), s) == _lib.DIB_EINVAL
    assert run(None, None, None, 8, 3, bias.data_ptr(), work.data_ptr(), s) == _lib.DIB_EINVAL
    assert b"null pointer" in l.dib_last_error()
    assert run(grad.data_ptr(), None, None, 8, 3, bias.data_ptr(), None, s) == _lib.DIB_EINVAL
    torch.cuda.synchronize()
    assert l.dib_device_status(0) == 0


# ---- the network -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny():
    """The fp32 test's network and inputs; Half input levels, fp32 targets.  Shared, never written."""
    from detectinblur_amd.models import deblur
    from detectinblur_amd.models import deblur_train as DT
    torch.manual_seed(6)
    model = deblur.MSResNet(n_scales=2, n_resblocks=2, n_feats=8, kernel_size=5).cuda().to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(7)
    sharp = torch.rand(2, 3, 16, 16, generator=g)
    blurred = ((sharp + torch.roll(sharp, 1, 3) + torch.roll(sharp, 2, 2)) / 3).cuda()
    inputs = DT.patch_levels(blurred, 2, torch.float16)
    weights = [torch.randn(2, 3, 16 >> s, 16 >> s, generator=g).cuda() for s in range(2)]      # the G_s of the smooth loss
    return model, inputs, weights


def test_half_levels_are_the_pyramid_kernels(tiny):
    from detectinblur_amd.models import deblur_train as DT
    _, inputs, _ = tiny
    assert [tuple(l.shape) for l in inputs] == [(2, 6, 16, 16), (2, 3, 8, 8)]
    assert all(l.dtype == torch.float16 and l.is_contiguous(memory_format=torch.channels_last) for l in inputs)
    g = torch.Generator().manual_seed(7)
    sharp = torch.rand(2, 3, 16, 16, generator=g)
    blurred = ((sharp + torch.roll(sharp, 1, 3) + torch.roll(sharp, 2, 2)) / 3).cuda()
    l32 = DT.patch_levels(blurred, 2)
    assert torch.equal(inputs[0][:, :3].float(), l32[0][:, :3])               # level 0 holds integers minus 127.5: exact in Half
    # half(half(L) - 127.5): from 128 up the first rounding errs by at most 2^-4 and the difference is exact; below, each by at most 2^-5
    assert (inputs[1].float() - l32[1]).abs().max() <= 2.0 ** -4


def test_amp_forward_equals_its_restatement_bit_for_bit(fused, tiny):
    DT = fused
    model, inputs, _ = tiny
    with torch.no_grad():
        want = DT.forward_amp_restated(model, inputs)
    got = DT.msresnet_train_forward(model, inputs)
    assert model.last_path == "hip-amp"
    for s, (o, w) in enumerate(zip(got, want)):
        assert o.dtype == torch.float16 and o.shape == w.shape
        assert torch.equal(_bits(o.contiguous()), _bits(w.contiguous())), s
    assert all(torch.isfinite(o).all() for o in got)


def test_amp_gradients_against_float64_beside_autocast(fused, tiny):
    """Every parameter gradient of the Half HIP path and of the autocast path on this GPU against float64 CPU autograd of the same module,
    under the smooth loss sum_s (out_s.float() * G_s).sum() (the L1 sign would turn Half-sized differences into whole-sign flips).  The
    HIP path rounds `half(conv) + b` to Half once more per convolution than autocast's convolution with bias does: that can double a
    layer's rounding error, not quadruple the total, so its worst relative error may be at most 4 x the autocast path's."""
    DT = fused
    model, inputs, weights = tiny

    def grads(net, ins, ws):
        for p in net.parameters():
            p.grad = None
        outs = DT.msresnet_train_forward(net, ins)
        sum((o.to(w.dtype) * w).sum() for o, w in zip(outs, ws)).backward()
        return {k: p.grad.detach() for k, p in net.named_parameters()}

    ref = copy.deepcopy(model).cpu().double()
    g64 = grads(ref, [l[:, :3].cpu().double().contiguous() for l in inputs], [w.cpu().double() for w in weights])
    assert ref.last_path == "torch"
    g_hip = grads(model, inputs, weights)
    assert model.last_path == "hip-amp"
    assert set(g_hip) == set(g64) and all(v.dtype == torch.float32 and torch.isfinite(v).all() for v in g_hip.values())
    g_hip = {k: v.double().cpu() for k, v in g_hip.items()}
    DT.FUSE_DEBLUR_TRAIN = False
    g_auto = {k: v.double().cpu() for k, v in grads(model, inputs, weights).items()}
    assert model.last_path == "torch-amp"

    def worst(gs):
        return max(float((gs[k] - g64[k]).abs().max() / g64[k].abs().max()) for k in g64)

    e_hip, e_auto = worst(g_hip), worst(g_auto)
    print("worst relative gradient error against float64 under --amp: hip-amp %.3e, torch-amp (autocast) %.3e" % (e_hip, e_auto))
    assert e_hip <= 4 * e_auto


# ---- end to end ------------------------------------------------------------------------------------------------------------------

def _drive(out_dir, *extra):
    from detectinblur_amd import train_deblurrer as TD
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        trainer = TD.main(["--synthetic", "--synthetic_images", "6", "--synthetic_size", "72", "88", "--device", "cuda", "-j", "0", "-b", "2",
                           "--patch_size", "16", "--print_freq", "1", "--epochs", "1", "--early_stop", "2", "--param_index", "1",
                           "--output_dir", str(out_dir), "--amp"] + TINY + list(extra))
    return buf.getvalue(), trainer


def test_amp_driver_trains_on_the_gpu_into_the_inference_stage(fused, tmp_path):
    from detectinblur_amd import _lib
    from detectinblur_amd import train_deblurrer as TD
    from detectinblur_amd.models import deblur
    text, trainer = _drive(tmp_path / "a")
    losses = [float(v) for v in re.findall(r"loss: ([0-9.einfa+-]+)", text)]
    assert len(losses) == 3 and all(np.isfinite(losses)), text[-2000:]
    assert text.count("path: hip-amp") == 3 and len(re.findall(r"scale: [0-9.e+]+", text)) == 3 and "3 steps, 6 images, 0 left out" in text
    assert trainer.optimizer._step_supports_amp_scaling and trainer.scaler.get_scale() == 1024.0
    with contextlib.redirect_stdout(io.StringIO()):
        d = deblur.Deblurer(str(tmp_path / "a"), device="cuda")
    out = d.deblur_(torch.rand(3, 20, 28, device="cuda"))
    assert d.last_path == "hip" and out.shape == (3, 20, 28) and torch.isfinite(out).all()
    torch.cuda.synchronize()
    assert _lib.lib().dib_device_status(0) == 0
    trained = torch.load(tmp_path / "a" / "models" / "model-1.pt", map_location="cpu", weights_only=True)["G"]
    assert all(v.dtype == torch.float32 for v in trained.values())
    # a scale of 2^60: every gradient overflows Half, every step is skipped, the weights stay; Half infinities are values, not faults
    text, trainer = _drive(tmp_path / "b", "--init_scale", "1152921504606846976")
    losses = [float(v) for v in re.findall(r"loss: ([0-9.einfa+-]+)", text)]
    assert len(losses) == 3 and all(np.isfinite(losses)) and text.count("path: hip-amp") == 3
    assert trainer.scaler.get_scale() == 2.0 ** 57
    args = TD.build_parser().parse_args(["--synthetic", "--device", "cuda", "--amp"] + TINY)
    args.distributed = False
    fresh = TD.Trainer(args, torch.device("cuda")).bare.state_dict()
    kept = torch.load(tmp_path / "b" / "models" / "model-1.pt", map_location="cpu", weights_only=True)["G"]
    assert all(torch.equal(kept[k], fresh[k].cpu()) for k in fresh)
    assert any(not torch.equal(trained[k], kept[k]) for k in kept)             # ... and at the default scale they do move
    torch.cuda.synchronize()
    assert _lib.lib().dib_device_status(0) == 0
