"""The fused squint warp on the GPU (csrc/dib_warp.hip behind `Warper(fused=True)`).  Reference everywhere: torch's float64
`grid_sample` on the CPU, fed the reference's Half grid `F.affine_grid(m).float().half()` -- what the reference's warper samples
at, with the sampling itself free of rounding.

Forward tolerance per element: 2^-21 * max|x| + 2^-22 * max(H, W) * D, D the largest difference between adjacent input pixels:
four float32 products and sums of values up to max|x| (first term), and the float32 rounding of the un-normalised coordinates,
at most 2^-22 * max(H, W) pixels, each pixel of offset moving the result by at most D (second term).
Backward tolerance per element: 2^-20 * max|g| + 2^-22 * max(H, W) * max|g|: a handful of float32 contributions summed by
atomic adds, and the same coordinate rounding acting on the weights."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen_goldens as GG
from detectinblur_amd.models import warper as WP

pytestmark = pytest.mark.gpu


def _params(inverse):
    _, _, th, l1, l2 = GG.warper_inputs()
    return (th, 1 / l1, 1 / l2) if inverse else (th, l1, l2)


def _matrices(shape, inverse):
    """The Half matrices as the fused path computes them (on the GPU), on the CPU."""
    th, l1, l2 = _params(inverse)
    return WP.squint_matrices(th.cuda(), l1.cuda(), l2.cuda(), shape[-1], shape[-2]).cpu()


def _half_grid(m, shape):
    return F.affine_grid(theta=m, size=shape, align_corners=False).float().half()


def _ref64(x, m):
    return F.grid_sample(x.double(), _half_grid(m, x.shape).double(), mode="bilinear", padding_mode="zeros", align_corners=False)


def _forward_tol(x):
    H, W = x.shape[-2:]
    D = max(float((x[..., 1:, :] - x[..., :-1, :]).abs().max()), float((x[..., :, 1:] - x[..., :, :-1]).abs().max()))
    return 2.0 ** -21 * float(x.abs().max()) + 2.0 ** -22 * max(H, W) * D


def _on_gpu(x, channels_last):
    xg = x.cuda()
    return xg.contiguous(memory_format=torch.channels_last) if channels_last else xg.contiguous()


def _fused(x, inverse, channels_last, requires_grad=False):
    th, l1, l2 = _params(inverse)
    w = WP.Warper(fused=True)
    xg = _on_gpu(x, channels_last).requires_grad_(requires_grad)
    assert w.takes_fused(xg)
    out = w(xg, th.cuda(), l1.cuda(), l2.cuda())
    assert out.dtype == torch.float32 and out.shape == x.shape
    assert out.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    return xg, out


def _seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


FORWARD_CASES = {
    "c8_10x14_nhwc_inverse": (lambda: GG.warper_inputs()[1], True, True),            # four channels per lane, the golden feature
    "c3_40x56_nhwc": (lambda: GG.warper_inputs()[0], False, True),                   # the image: one lane per pixel
    "c3_40x56_planar": (lambda: GG.warper_inputs()[0], False, False),
    "c256_25x42_nhwc": (lambda: _seeded((3, 256, 25, 42), 5), False, True),           # one wave per pixel, odd height
    "c6_10x14_nhwc": (lambda: _seeded((3, 6, 10, 14), 6), False, True),               # C % 4 != 0
    "c8_7x11_nhwc": (lambda: _seeded((3, 8, 7, 11), 7), False, True),                 # a row narrower than a wave
    "c3_7x11_planar_inverse": (lambda: _seeded((3, 3, 7, 11), 8), True, False),
}


@pytest.mark.parametrize("case", list(FORWARD_CASES))
def test_forward_matches_float64_sampling_of_the_half_grid(case):
    make, inverse, channels_last = FORWARD_CASES[case]
    x = make()
    ref = _ref64(x, _matrices(x.shape, inverse))
    _, out = _fused(x, inverse, channels_last)
    err = float((out.cpu().double() - ref).abs().max())
    tol = _forward_tol(x)
    outside = float((_half_grid(_matrices(x.shape, inverse), x.shape).abs() > 1.0).any(dim=-1).float().mean())
    print("%s: max err %.3e, tolerance %.3e, samples outside [-1, 1]: %.1f %%" % (case, err, tol, 100 * outside))
    assert inverse or outside > 0.03            # the zero-padding branches are exercised
    assert err <= tol                           # every output element


@pytest.mark.parametrize("channels_last", [True, False], ids=["nhwc", "planar"])
def test_ramps_expose_the_sampling_positions(channels_last):
    """Channels j / (W - 1) and i / (H - 1) at 8 x 1344: the output IS the sampling position (where all four corners are inside).
    One Half ulp of a grid coordinate near +-1 is 2^-11 * 1344 / 2 = 0.33 px = 2.4e-4 of the x ramp; the tolerance is ~7e-7."""
    H, W = 8, 1344
    x = torch.stack((torch.arange(W, dtype=torch.float32).div(W - 1).expand(H, W),
                     torch.arange(H, dtype=torch.float32).div(H - 1)[:, None].expand(H, W)))[None].repeat(3, 1, 1, 1).contiguous()
    m = _matrices(x.shape, False)
    ref = _ref64(x, m)
    _, out = _fused(x, False, channels_last)
    # per channel: D is 1 / (W - 1) for the x ramp and 1 / (H - 1) for the y ramp
    err = [float((out.cpu().double() - ref)[:, c].abs().max()) for c in (0, 1)]
    tol = [_forward_tol(x[:, c:c + 1]) for c in (0, 1)]
    # the sensitivity claimed above, on this very reference: the grid moved by one Half ulp
    g = _half_grid(m, x.shape)
    moved = (g.view(torch.int16) + 1).view(torch.float16)
    shifted = F.grid_sample(x.double(), moved.double(), mode="bilinear", padding_mode="zeros", align_corners=False)
    inside = (g.abs() < 0.9).all(dim=-1)
    ulp = float((shifted - ref)[:, 0][inside].abs().max())
    print("ramps: max err x %.3e y %.3e, tolerance x %.3e y %.3e, one Half ulp moves the x ramp by up to %.3e" % (err[0], err[1], tol[0], tol[1], ulp))
    assert tol[0] < 1e-6 and ulp > 1e-4
    assert err[0] <= tol[0] and err[1] <= tol[1]


def test_existing_contract_against_the_reference_goldens(golden):
    """tests/test_warper.py's tolerances for torch's Half kernels on the GPU, met by the fused path (float32 sampling of the same
    Half grid; on the CPU that arithmetic measures 3.8e-2 / 2.3e-3 and 5.4e-4 / 7.1e-3)."""
    x = GG.warper_inputs()[0]
    d = np.abs(_fused(x, False, False)[1].cpu().numpy() - golden.warper["warp_image"])
    print("warp_image: max %.3e mean %.3e" % (d.max(), d.mean()))
    assert d.max() <= 5e-2 and d.mean() <= 5e-3
    f = GG.warper_inputs()[1]
    d = np.abs(_fused(f, True, True)[1].cpu().numpy() - golden.warper["warp_feature"])
    print("warp_feature: max %.3e mean %.3e" % (d.max(), d.mean()))
    d = np.abs(_fused(GG.warper_smooth_input(), False, False)[1].cpu().numpy() - golden.warper["warp_smooth"])
    print("warp_smooth: mean %.3e p99 %.3e" % (d.mean(), np.percentile(d, 99)))
    assert d.mean() <= 1.5e-3 and np.percentile(d, 99) <= 1.5e-2


@pytest.mark.parametrize("channels_last", [True, False], ids=["nhwc", "planar"])
def test_nan_and_inf_pixels_reach_the_outputs_torch_lets_them_reach(channels_last):
    x = GG.warper_inputs()[0].clone()
    x[0, 1, 20, 30] = float("nan")
    x[1, 0, 10, 12] = float("inf")
    ref = _ref64(x, _matrices(x.shape, False))
    out = _fused(x, False, channels_last)[1].cpu()
    assert int(torch.isnan(ref).sum()) >= 2 and int(torch.isinf(ref).sum()) >= 2
    assert torch.equal(torch.isnan(out), torch.isnan(ref))
    assert torch.equal(torch.isinf(out), torch.isinf(ref)) and torch.equal(out[torch.isinf(ref)] > 0, ref[torch.isinf(ref)] > 0)
    finite = torch.isfinite(ref)
    assert float((out.double() - ref)[finite].abs().max()) <= _forward_tol(GG.warper_inputs()[0])


BACKWARD_CASES = {
    "c8_10x14_nhwc_inverse": (lambda: GG.warper_inputs()[1], True, True),
    "c256_25x42_nhwc_inverse": (lambda: _seeded((3, 256, 25, 42), 5), True, True),
    "c3_7x11_planar": (lambda: _seeded((3, 3, 7, 11), 8), False, False),
}


@pytest.mark.parametrize("case", list(BACKWARD_CASES))
def test_backward_matches_float64_autograd(case):
    make, inverse, channels_last = BACKWARD_CASES[case]
    x = make()
    g = _seeded(x.shape, 21)
    x64 = x.double().requires_grad_(True)
    F.grid_sample(x64, _half_grid(_matrices(x.shape, inverse), x.shape).double(), mode="bilinear", padding_mode="zeros",
                  align_corners=False).backward(g.double())
    xg, out = _fused(x, inverse, channels_last, requires_grad=True)
    out.backward(_on_gpu(g, channels_last))
    got = xg.grad.cpu()
    H, W = x.shape[-2:]
    tol = (2.0 ** -20 + 2.0 ** -22 * max(H, W)) * float(g.abs().max())
    err = float((got.double() - x64.grad).abs().max())
    zeros = x64.grad == 0
    print("%s: max err %.3e, tolerance %.3e, %d of %d input gradients are zero in the reference" % (case, err, tol, int(zeros.sum()), zeros.numel()))
    assert err <= tol
    assert bool((got[zeros] == 0).all())


def test_no_backward_launch_for_an_input_without_gradient(monkeypatch):
    calls = []
    real = WP._SquintWarp.backward
    monkeypatch.setattr(WP._SquintWarp, "backward", staticmethod(lambda ctx, g: calls.append(1) or real(ctx, g)))
    feat = GG.warper_inputs()[1]
    xg, out = _fused(feat, True, True, requires_grad=True)
    out.sum().backward()
    assert calls == [1] and xg.grad is not None                 # the counter sees a backward pass that does run
    # the image warp: its input needs no gradient, something downstream does
    scale = torch.ones((), device="cuda", requires_grad=True)
    xg, out = _fused(GG.warper_inputs()[0], False, True)
    assert not out.requires_grad and out.grad_fn is None
    (out * scale).sum().backward()
    assert calls == [1] and scale.grad is not None


def test_no_fused_warp_switch_takes_the_torch_path(monkeypatch):
    x = GG.warper_inputs()[0].cuda()
    w = WP.Warper(fused=True)
    th, l1, l2 = (t.cuda() for t in _params(False))
    assert w.takes_fused(x) and not w.takes_fused(x.half()) and not w.takes_fused(x[:, :, ::2]) and not WP.Warper().takes_fused(x)
    monkeypatch.setenv("DIB_NO_FUSED_WARP", "1")
    assert not w.takes_fused(x)
    assert torch.equal(w(x, th, l1, l2), WP.Warper()(x, th, l1, l2))


# ---- inside the detector ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """tests/_squint_warp_children.py, once for the module: the torch-path training step (DIB_NO_FUSED_WARP=1) and the graphed
    warped trunk in MIOpen's deterministic mode."""
    from detectinblur_amd import utils
    from tests import _squint_warp_children as children
    ctx = utils.loader_context()
    if ctx is None:
        pytest.skip("no fork server (the GPU was initialised before the test session could start one)")
    out = str(tmp_path_factory.mktemp("squint") / "child.json")
    p = ctx.Process(target=children.detector_without_fused_warp_then_graphed, args=(out,))
    p.start()
    p.join(600)
    if p.is_alive():
        p.kill()
        p.join()
        pytest.fail("child timed out")
    if os.path.exists(out + ".err"):
        pytest.fail(open(out + ".err").read()[-4000:])
    assert p.exitcode == 0 and os.path.exists(out), p.exitcode
    r = json.load(open(out))
    print(json.dumps(r))
    return r


def test_fused_warps_inside_the_training_detector(child):
    """Two ragged images through the training detector: the six warper calls (the image, five pyramid levels) each match the
    float64 reference of their own recorded input; losses are finite; every trunk parameter the torch-path warper hands a
    gradient to (child process, DIB_NO_FUSED_WARP=1) gets a finite, non-zero one through the fused backward pass."""
    from tests._squint_warp_children import toy_batch, toy_detector
    m = toy_detector().train()
    imgs, tg, (th, l1, l2) = toy_batch()
    calls = []
    m.warper.register_forward_hook(lambda mod, args, out: calls.append(tuple(a.detach().cpu() for a in args) + (out.detach().cpu(), m.warper.takes_fused(args[0]))))
    losses = m(imgs, tg, thetas=th, lambda1s=l1, lambda2s=l2)
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    sum(losses.values()).backward()
    assert len(calls) == 6 and all(c[5] for c in calls)
    assert [c[0].shape[1] for c in calls] == [3] + [256] * 5
    for x, t, a, b, out, _ in calls:
        mats = WP.squint_matrices(t.cuda(), a.cuda(), b.cuda(), x.shape[-1], x.shape[-2]).cpu()
        err, tol = float((out.double() - _ref64(x, mats)).abs().max()), _forward_tol(x)
        print("warper call %s: max err %.3e, tolerance %.3e" % (tuple(x.shape), err, tol))
        assert err <= tol
    assert torch.equal(calls[1][2], 1 / l1.cpu()) and torch.equal(calls[0][2], l1.cpu())
    names = child["trunk_grads_torch_path"]
    assert len(names) > 20
    grads = dict(m.backbone.named_parameters())
    for n in names:
        g = grads[n].grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, n


def test_captured_trunk_reads_its_matrices_at_replay(child):
    """graph_inference on a warping detector: once the warped trunk is captured, calls with a second and a third
    (theta, l1, l2) replay the SAME graph and equal eager fused inference with those parameters bit for bit (boxes, labels,
    scores) -- a graph that had baked the first matrices in would return the first result three times."""
    assert child["eager_reproducible"]                       # the yardstick: eager inference equals itself in this mode
    assert child["captured"] and child["still_one_graph"] and not child["plain_trunk_cache_used"]
    assert min(child["detections"]) > 0
    assert child["sets_differ"] == [True, True, True]
    assert child["replay_equals_eager"] == [True, True, True, True]
