"""The DeepDeblur trainer without a GPU: the draw order and the patch geometry against the reference's dataCommon.py (which imports
scikit-image and cannot be imported here: its order is restated below with line citations), the torch restatements of the two
reduction kernels against float64 definitions, the torch path of the network, and the driver end to end on the CPU."""
import contextlib
import io
import os
import random

import numpy as np
import pytest
import torch

from detectinblur_amd import train_deblurrer as TD
from detectinblur_amd.models import deblur
from detectinblur_amd.models import deblur_train as DT

TINY = ["--n_scales", "2", "--n_resblocks", "2", "--n_feats", "8", "--kernel_size", "5"]


# ---- dataCommon.py, restated ------------------------------------------------------------------------------------------------------

def _datacommon_draws(h, w, ps):
    py = random.randrange(0, h - ps + 1)            # crop :32
    px = random.randrange(0, w - ps + 1)            # crop :33
    choices = (False, True)                         # augment :59
    hflip = random.choice(choices)                  # :61
    vflip = random.choice(choices)                  # :62
    rot90 = random.choice(choices)                  # :63
    rgb_order = list(range(3))                      # :67
    random.shuffle(rgb_order)                       # :68
    return py, px, hflip, vflip, rot90, rgb_order


def _datacommon_patch(img, py, px, ps, hflip, vflip, rot90, rgb_order):
    """img: H x W x 3, as dataCommon handles it"""
    img = img[py:py + ps, px:px + ps, :]            # _crop :39
    if hflip:
        img = img[:, ::-1, :]                       # _augment :76
    if vflip:
        img = img[::-1, :, :]                       # :77
    if rot90:
        img = img.transpose(1, 0, 2)                # :78
    return img[..., rgb_order]                      # :81 (the identity order indexes the same values)


@pytest.mark.parametrize("seed", [0, 1, 7, 1337])
def test_draw_order_is_datacommons(seed):
    random.seed(seed)
    want = [_datacommon_draws(40, 56, 16), _datacommon_draws(16, 16, 16)]
    after = random.random()
    random.seed(seed)
    got = [DT.draw_patch(40, 56, 16), DT.draw_patch(16, 16, 16)]
    assert random.random() == after                 # the same number of draws was consumed
    for w, g in zip(want, got):
        assert (g.py, g.px, g.hflip, g.vflip, g.rot90, list(g.order)) == w


def test_patch_gather_equals_numpy_slicing_in_datacommons_order():
    rs = np.random.RandomState(0)
    images = [rs.random_sample((3, 20, 28)).astype(np.float32), rs.random_sample((3, 17, 40)).astype(np.float32)]
    ps = 12
    for order in ((2, 0, 1), (0, 1, 2), (1, 0, 2)):
        for bits in range(8):
            hflip, vflip, rot90 = bool(bits & 1), bool(bits & 2), bool(bits & 4)
            draws = [DT.PatchDraw(3, 5, hflip, vflip, rot90, order), DT.PatchDraw(5, 28, hflip, vflip, rot90, order)]
            got = DT.gather_patches([torch.from_numpy(a) for a in images], draws, ps).numpy()
            for b, (a, d) in enumerate(zip(images, draws)):
                want = _datacommon_patch(a.transpose(1, 2, 0), d.py, d.px, ps, hflip, vflip, rot90, list(order)).transpose(2, 0, 1)
                assert np.array_equal(got[b], want), (order, bits, b)
            w = DT.flags_word(draws[0])
            assert (w & 7) == bits and [(w >> 4) & 3, (w >> 6) & 3, (w >> 8) & 3] == list(order)


# ---- the two reductions, restated in torch, against float64 ---------------------------------------------------------------------

def test_bias_grad_restatement_against_float64():
    g = torch.Generator().manual_seed(1)
    n_pix, C = 37, 8
    y = torch.randn(n_pix, C, generator=g)
    y[3, 2] = float("nan")                          # a NaN activation carries no mask bit
    y[4, 1] = 0.0
    grad = torch.randn(n_pix, C, generator=g)
    grad[5, 3], grad[6, 6] = float("nan"), float("inf")
    y[5, 3], y[6, 6] = 1.0, 2.0                     # both pass the mask
    grad[7, 0], y[7, 0] = float("nan"), -1.0        # this one is masked away
    mask = DT.sign_mask_torch(y)
    assert mask.dtype == torch.uint8 and mask.numel() == n_pix * C // 4
    out, bias = DT.bias_grad_torch(grad, mask)
    want = torch.where(y > 0, grad.double(), torch.zeros((), dtype=torch.float64))
    assert torch.equal(out.double().nan_to_num(nan=-7.0), want.nan_to_num(nan=-7.0))
    assert out[3, 2] == 0 and out[4, 1] == 0 and out[7, 0] == 0
    want_bias = want.sum(0)
    poisoned = [3, 6]                               # the NaN and the inf reach their own channel's sum and no other
    assert torch.isnan(bias[3]) and torch.isinf(bias[6])
    clean = [c for c in range(C) if c not in poisoned]
    assert torch.isfinite(bias[clean]).all()
    bound = n_pix * 2.0 ** -24 * want.abs().sum(0)[clean]
    assert ((bias[clean].double() - want_bias[clean]).abs() <= bound).all()
    # without a mask: the plain channel sum, any C
    out3, bias3 = DT.bias_grad_torch(grad[:, :3])
    assert out3.data_ptr() == grad[:, :3].data_ptr() and torch.allclose(bias3[1:3], grad[:, 1:3].sum(0))


def test_l1_level_restatement_against_float64():
    g = torch.Generator().manual_seed(2)
    n_pix = 29
    out = torch.randn(n_pix, 3, generator=g) * 50
    target = torch.randn(n_pix, 6, generator=g) * 50
    target[2, 1] = out[2, 1]                        # d == +0
    out[3, 0], target[3, 0] = -0.0, 0.0             # d == -0
    grad, term = DT.l1_level_torch(out, target, 1.0)
    d = out.double() - target[:, :3].double()
    k = np.float32(1.0) / np.float32(3 * n_pix)
    assert grad[2, 1] == 0 and grad[3, 0] == 0
    assert set(np.unique(grad.numpy()).tolist()) == {float(-k), 0.0, float(k)}
    assert torch.equal(grad.double(), torch.sign(d) * float(k))
    want = d.abs().sum() / (3 * n_pix)
    assert abs(term.double() - want) <= (3 * n_pix + 2) * 2.0 ** -24 * float(want)
    out[4, 2] = float("nan")
    grad, term = DT.l1_level_torch(out, target, 1.0)
    assert torch.isnan(grad[4, 2]) and torch.isnan(term) and torch.isfinite(grad).sum() == 3 * n_pix - 1
    # torch's own l1_loss backward agrees everywhere else; at the NaN its sign() is 0 and hides it, which the kernel does not copy
    o = out.clone().requires_grad_(True)
    torch.nn.functional.l1_loss(o, target[:, :3]).backward()
    assert torch.allclose(o.grad, grad.nan_to_num(nan=0.0), rtol=1e-6, atol=0)


def test_depth_formulas_of_the_summation_trees():
    # csrc/dib_deblur_train.hip, "THE SUMMATION ORDER": L + ceil(log2 R) + S - 1
    assert DT.bias_grad_depth(1, 64) == 1 + 4 + 0                   # R = 16 rows, one slice, one pixel
    assert DT.bias_grad_depth(4099, 64) == 16 + 4 + 16              # S = ceil(4099 / 256) = 17 slices of <= 242 pixels: L = 16
    assert DT.bias_grad_depth(257, 3) == 4 + 7 + 0                  # R = 85 rows, one slice: L = ceil(257 / 85)
    assert DT.bias_grad_depth(16 * 256 * 256, 64) == 64 + 4 + 1023  # the trainer's default level 0
    assert DT.l1_loss_depth(1) == 1 + 8 + 0
    assert DT.l1_loss_depth(1027) == 7 + 8 + 1                      # 3081 elements: 2 slices of <= 1541: L = 7


# ---- the network's torch path ---------------------------------------------------------------------------------------------------

def _tiny(seed=0):
    torch.manual_seed(seed)
    return deblur.MSResNet(n_scales=2, n_resblocks=2, n_feats=8, kernel_size=5)


def test_levels_and_torch_forward_are_the_inference_stages():
    model = _tiny()
    g = torch.Generator().manual_seed(3)
    patches = torch.rand(2, 3, 16, 16, generator=g)
    levels = DT.patch_levels(patches, 2)
    assert [tuple(l.shape) for l in levels] == [(2, 6, 16, 16), (2, 3, 8, 8)]
    for b in range(2):
        for l, want in zip(levels, deblur.pyramid(deblur.quantise(patches[b]), 2)):
            assert torch.equal(l[b, :3], want - 127.5)
    out = DT.msresnet_train_forward(model, levels)
    assert model.last_path == "torch"
    want = model([l[:, :3] + 127.5 for l in levels])
    for o, w in zip(out, want):
        assert torch.allclose(o + 127.5, w, rtol=0, atol=1e-4)
    with pytest.raises(ValueError):
        DT.patch_levels(torch.rand(1, 3, 6, 6), 3)


def test_tiny_net_overfits_one_batch():
    model = _tiny(1)
    g = torch.Generator().manual_seed(4)
    sharp = torch.rand(2, 3, 16, 16, generator=g)
    blurred = (sharp + torch.roll(sharp, 1, 3) + torch.roll(sharp, 1, 2)) / 3
    inputs, targets = DT.patch_levels(blurred, 2), DT.patch_levels(sharp, 2)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(40):
        loss = DT.pyramid_l1_loss(DT.msresnet_train_forward(model, inputs), targets)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], (losses[0], losses[-1])


# ---- the driver -----------------------------------------------------------------------------------------------------------------

def _run(out_dir, *extra):
    argv = ["--synthetic", "--synthetic_images", "4", "--synthetic_size", "40", "56", "--device", "cpu", "-j", "0", "-b", "2",
            "--patch_size", "16", "--print_freq", "1", "--output_dir", str(out_dir)] + TINY + list(extra)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        TD.main(argv)
    return buf.getvalue()


def test_checkpoint_round_trip_into_the_inference_stage(tmp_path):
    text = _run(tmp_path, "--epochs", "1", "--early_stop", "0", "--validate_images", "1")
    assert "path: torch" in text and "0 left out" in text and "Validation: [1]  PSNR deblurred" in text
    assert sorted(os.listdir(tmp_path / "models")) == ["model-1.pt"]            # no optimizer file beside it
    assert sorted(os.listdir(tmp_path / "optim")) == ["optim-1.pt"]
    state = torch.load(tmp_path / "models" / "model-1.pt", map_location="cpu", weights_only=True)
    assert set(state) == {"G"}
    with contextlib.redirect_stdout(io.StringIO()):
        d = deblur.Deblurer(str(tmp_path))                                     # strict load
    assert (d.model.n_scales, d.model.n_resblocks, d.model.n_feats, d.model.kernel_size) == (2, 2, 8, 5)
    out = d.deblur_(torch.rand(3, 20, 28))
    assert out.shape == (3, 20, 28) and torch.isfinite(out).all()


def test_resume_gives_the_weights_of_the_uninterrupted_run(tmp_path):
    _run(tmp_path / "a", "--epochs", "2", "--save_every", "1")
    _run(tmp_path / "b", "--epochs", "1", "--save_every", "1")
    text = _run(tmp_path / "b", "--epochs", "2", "--save_every", "1", "--resume")
    assert "Resumed from" in text and "Epoch: [2]" in text and "Epoch: [1]" not in text
    a = torch.load(tmp_path / "a" / "models" / "model-2.pt", weights_only=True)["G"]
    b = torch.load(tmp_path / "b" / "models" / "model-2.pt", weights_only=True)["G"]
    first = torch.load(tmp_path / "a" / "models" / "model-1.pt", weights_only=True)["G"]
    assert set(a) == set(b)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(a[k], first[k]) for k in a)                     # the second epoch did train


def test_small_images_are_left_out_and_counted(tmp_path):
    text = _run(tmp_path, "--epochs", "1", "--patch_size", "48")              # 40 x 56 images: every one is too small
    assert "4 images, 4 left out" in text


def test_refusals_and_the_string_sort_warning(tmp_path, capsys):
    with pytest.raises(SystemExit, match="cpu_blur"):
        TD.main(["--synthetic", "--cpu_blur"])
    with pytest.raises(SystemExit, match="multiple of 2"):
        TD.main(["--synthetic", "--patch_size", "18", "--n_scales", "3"])
    models = tmp_path / "models"
    models.mkdir()
    assert not TD.warn_if_not_picked(str(models), 9)
    (models / "model-9.pt").write_bytes(b"")
    assert TD.warn_if_not_picked(str(models), 10)                              # "model-9.pt" sorts after "model-10.pt"
    assert "model-10.pt is written" in capsys.readouterr().out
    assert deblur.find_checkpoint(str(tmp_path)).endswith("model-9.pt")        # ... and that is what the inference stage picks
