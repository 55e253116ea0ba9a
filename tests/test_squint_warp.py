"""The fused squint warp (`Warper(fused=True)`, csrc/dib_warp.hip), the parts that need no GPU: the coordinate arithmetic the kernel
implements, stated as torch code (`squint_half_grid`), equals torch's own Half affine_grid bit for bit; the torch path is what it
was; the new entry points reject bad arguments before any device call; the detector builds the fused warper."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen_goldens as GG
from detectinblur_amd.models import warper as WP

SIZES = [(40, 56), (10, 14), (7, 11), (25, 42), (8, 1344)]


@pytest.mark.parametrize("inverse", [False, True], ids=["l1_l2", "inverse_l1_l2"])
@pytest.mark.parametrize("H,W", SIZES)
def test_half_grid_arithmetic_equals_torch_affine_grid_bit_for_bit(H, W, inverse):
    _, _, th, l1, l2 = GG.warper_inputs()
    if inverse:
        l1, l2 = 1 / l1, 1 / l2
    m = WP.squint_matrices(th, l1, l2, W, H)
    want = F.affine_grid(theta=m, size=(m.shape[0], 1, H, W), align_corners=False).float().half()
    got = WP.squint_half_grid(m, H, W)
    assert got.dtype == torch.float16 and got.shape == want.shape
    assert np.array_equal(got.numpy().view(np.uint16), want.numpy().view(np.uint16))
    # the comparison can fail: the closed form of the base coordinates, rounded to Half once, is NOT torch's base grid
    if W == 1344:
        closed = ((2 * torch.arange(W, dtype=torch.float64) + 1) / W - 1).half()
        assert (closed != WP.squint_base_grid(H, W)[0]).sum() > 100


@pytest.mark.parametrize("H,W", SIZES)
def test_base_grid_is_torchs_own_expression(H, W):
    bx, by = WP.squint_base_grid(H, W)
    assert bx.dtype == by.dtype == torch.float16 and bx.shape == (W,) and by.shape == (H,) and bx.device.type == "cpu"
    # independent of the expression in warper.py: the Half identity matrix makes affine_grid return its base grid
    eye = torch.tensor([[[1.0, 0, 0], [0, 1.0, 0]]]).half()
    g = F.affine_grid(eye, (1, 1, H, W), align_corners=False)
    assert torch.equal(g[0, 0, :, 0], bx) and torch.equal(g[0, :, 0, 1], by)
    assert torch.equal(bx, torch.linspace(-1, 1, W, dtype=torch.float16) * (W - 1) / W)
    assert WP.squint_base_grid(H, W)[0] is bx                    # cached per geometry and device


def test_base_grid_of_a_one_pixel_axis_is_zero():
    # torch's linspace_from_neg_one returns 0 for a single step (its Half CPU kernel does not exist: asked in float32)
    g = F.affine_grid(torch.tensor([[[1.0, 0, 0], [0, 1.0, 0]]]), (1, 1, 1, 5), align_corners=False)
    assert float(g[0, 0, 0, 1]) == 0.0
    bx, by = WP.squint_base_grid(1, 5)
    assert by.tolist() == [0.0] and bx.shape == (5,)


def test_fused_warper_on_cpu_tensors_is_the_torch_path(golden):
    x, feat, th, l1, l2 = GG.warper_inputs()
    w = WP.Warper(fused=True)
    assert not w.takes_fused(x)
    assert np.array_equal(w(x, th, l1, l2).numpy(), golden.warper["warp_image"])
    assert np.array_equal(w(feat, th, 1 / l1, 1 / l2).numpy(), golden.warper["warp_feature"])
    assert np.array_equal(w(GG.warper_smooth_input(), th, l1, l2).numpy(), golden.warper["warp_smooth"])


def test_argument_errors_are_reported_without_a_gpu():
    from detectinblur_amd import _lib
    l = _lib.lib()
    p = 4096                       # any non-null value: every case below is rejected before a pointer is used
    for fn in (l.dib_squint_warp_forward, l.dib_squint_warp_backward):
        name = fn.__name__.encode()
        assert fn(None, p, 1, 4, 8, 8, _lib.DIB_WARP_NHWC, p, p, p, None) == _lib.DIB_EINVAL
        assert name in l.dib_last_error() and b"null pointer" in l.dib_last_error()
        for missing in range(3):
            tail = [p, p, p]
            tail[missing] = None
            assert fn(p, 2 * p, 1, 4, 8, 8, _lib.DIB_WARP_NCHW, *tail, None) == _lib.DIB_EINVAL
            assert b"null pointer" in l.dib_last_error()
        for shape in ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, -3, 8), (1, 4, 8, 0)):
            assert fn(p, 2 * p, *shape, _lib.DIB_WARP_NHWC, p, p, p, None) == _lib.DIB_EINVAL
            assert b"> 0" in l.dib_last_error()
        assert fn(p, 2 * p, 1, 4, 8, 8, 2, p, p, p, None) == _lib.DIB_EINVAL
        assert b"unknown layout 2" in l.dib_last_error()
        assert fn(p, 2 * p, 70000, 256, 70000, 8, _lib.DIB_WARP_NHWC, p, p, p, None) == _lib.DIB_EINVAL
        assert b"too large" in l.dib_last_error()
        assert fn(p, p, 1, 4, 8, 8, _lib.DIB_WARP_NHWC, p, p, p, None) == _lib.DIB_EINVAL
        assert b"alias" in l.dib_last_error()


def test_detector_builds_the_fused_warper_and_the_default_stays_torch():
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    assert WP.Warper().fused is False
    m = fasterrcnn_resnet50_fpn(num_classes=5, pretrained=False, pretrained_backbone=False, warp_internally=True, min_size=96, max_size=128)
    assert m.warper.fused is True

