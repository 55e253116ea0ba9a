"""dib_deblur_patches_augment (csrc/dib_deblur_augment.hip) on the GPU: bit for bit against models/deblur_train.augment_patches_torch
without noise, element by element against a float64 HSV round trip plus the float64 normal of oracle/dib_oracle.py with noise, the
chunking across the 64-image launch limit, the identity through both pyramid kernels, the refusals, and the driver with
--change_saturation and --patch_noise_sigma."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import dib_oracle as O
from tests.test_deblur_augment import GRID_PS, TOL, colour_grid_levels, draws_of, grid_patches, saturation64, special_image
from tests.test_deblur_train import TINY
from tests.test_postops_reference import EPS_N

pytestmark = pytest.mark.gpu

SHAPES = [(3, 20, 28), (3, 17, 40), (3, 12, 12)]
FACTORS = (0.5, 1.0, 1.5)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _images(shapes, dtype, seed):
    """values between the levels, below 0 and above 1, with the special values of the CPU file in the first image"""
    g = torch.Generator().manual_seed(seed)
    images = [(torch.rand(s, generator=g) * 1.5 - 0.25).to(dtype) for s in shapes]
    images[0].view(-1)[:8] = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, -1.0, 1.0001, 2.5, 1e-8]).to(dtype)
    return images


# ---- sigma = 0: bit-equal to the restatement ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("corner", ["origin", "far"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("ps,shapes", [(12, SHAPES), (16, [(3, 16, 16), (3, 21, 16), (3, 16, 19)]), (20, [(3, 20, 28), (3, 23, 40), (3, 20, 20)])],
                         ids=["ps12", "ps16", "ps20"])
def test_bit_equal_to_the_restatement_without_noise(ps, shapes, dtype, corner):
    """ps 12: one partial workgroup; 16: exactly one; 20: two, the second partial."""
    from detectinblur_amd.models import deblur_train as DT
    images = _images(shapes, dtype, ps)
    dev = [im.cuda() for im in images]
    for order in ((2, 0, 1), (0, 1, 2)):
        for bits in range(8):
            draws = [draws_of(bits, order, 0 if corner == "origin" else s[1] - ps, 0 if corner == "origin" else s[2] - ps,
                              saturation=FACTORS[(b + bits) % 3], sigma=2.0, key=(b, 9)) for b, s in enumerate(shapes)]
            got = DT.augment_patches(dev, draws, ps, False)
            assert got.shape == (3, 3, ps, ps) and got.dtype == torch.float32 and got.is_cuda
            want_dev = DT.augment_patches_torch(dev, draws, ps, False)
            assert torch.equal(_bits(got), _bits(want_dev)), (order, bits)
            assert torch.equal(_bits(got.cpu()), _bits(DT.augment_patches_torch(images, draws, ps, False))), (order, bits)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_colour_grid_and_special_values_without_noise(dtype):
    from detectinblur_amd.models import deblur, deblur_train as DT
    images, origins = grid_patches(dtype)
    dev = [im.cuda() for im in images]
    arrays = colour_grid_levels()
    for a in FACTORS:
        draws = [draws_of(0, (0, 1, 2), 0, px, saturation=a) for _, px in origins]
        got = DT.augment_patches([dev[i] for i, _ in origins], draws, GRID_PS, True)
        want = DT.augment_patches_torch([images[i] for i, _ in origins], draws, GRID_PS, True)
        assert torch.equal(_bits(got.cpu()), _bits(want)), a
        # ... and the float64 HSV round trip of the levels the image holds (a Half image does not hold k / 255)
        q = [deblur.quantise(im).double().numpy() for im in images]
        if dtype == torch.float32:
            assert all(np.array_equal(x, y) for x, y in zip(q, arrays))
        x64 = np.stack([saturation64(q[i][:, :, px:px + GRID_PS], a) for i, px in origins])
        levels = np.rint(got.cpu().double().numpy() * 255.0)
        assert (np.abs(levels - x64) <= 0.5 + TOL).all(), (a, float(np.abs(levels - x64).max()))
    sp = [special_image(dtype, 0), special_image(dtype, 1)]
    for bits in range(8):
        draws = [draws_of(bits, (1, 2, 0), 4, 0, saturation=0.5), draws_of(bits, (0, 2, 1), 0, 4, saturation=1.5)]
        got = DT.augment_patches([im.cuda() for im in sp], draws, 16, True)
        assert torch.equal(_bits(got.cpu()), _bits(DT.augment_patches_torch(sp, draws, 16, True))), bits
        assert torch.isfinite(got).all()


# ---- with noise: against float64 ------------------------------------------------------------------------------------------------------

SIGMAS = (-3.1, 0.0, 0.4, 6.0)


def _noise_case(dtype):
    from detectinblur_amd.models import deblur_train as DT
    ps = 20
    shapes = [(3, 20, 28), (3, 23, 40), (3, 20, 20), (3, 31, 22)]
    images = _images(shapes, dtype, 11)
    draws = [draws_of(b + 3, ((2, 0, 1), (0, 1, 2))[b % 2], s[1] - ps, (s[2] - ps) // 2, saturation=(0.5, 1.0, 1.5, 1.23)[b], sigma=SIGMAS[b],
                      key=(1000 + b, 77 * b)) for b, s in enumerate(shapes)]
    return DT, ps, images, [im.cuda() for im in images], draws


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_noise_against_float64(dtype):
    from detectinblur_amd.models import deblur
    DT, ps, images, dev, draws = _noise_case(dtype)
    got = DT.augment_patches(dev, draws, ps, True)
    again = DT.augment_patches(dev, draws, ps, True)
    assert torch.equal(_bits(got), _bits(again))
    levels = np.rint(got.cpu().double().numpy() * 255.0)
    assert np.array_equal((levels / 255.0).astype(np.float32), got.cpu().numpy())
    index = np.arange(3 * ps * ps, dtype=np.uint64).reshape(3, ps, ps)                 # i = (c * ps + y) * ps + x of the OUTPUT patch
    for b, d in enumerate(draws):
        q = deblur.quantise(DT.gather_patches_torch([images[b]], [d], ps)[0]).double().numpy()
        sigma = float(np.float32(d.sigma))
        x64 = np.clip(saturation64(q, d.saturation) + sigma * O.normal64(index, d.key), 0.0, 255.0)
        err = np.abs(levels[b] - x64)
        print("image %d sigma %g: max |g - x64| = %.6f" % (b, d.sigma, err.max()))
        assert (err <= 0.5 + TOL + EPS_N * abs(sigma)).all(), (b, float(err.max()))
        if d.sigma != 0:
            assert float(np.abs(levels[b] - np.rint(saturation64(q, d.saturation))).max()) >= 1.0      # there is noise
    # noise=False is the sigma = 0 result
    clean = DT.augment_patches(dev, draws, ps, False)
    assert torch.equal(_bits(clean), _bits(DT.augment_patches(dev, [d._replace(sigma=0.0) for d in draws], ps, True)))
    assert torch.equal(_bits(clean[1]), _bits(got[1]))                                   # sigma[1] == 0
    # image b does not see another image's key or sigma
    others = [d if b == 2 else d._replace(sigma=d.sigma + 1.5, key=(d.key[0] ^ 0x55, d.key[1] + 1)) for b, d in enumerate(draws)]
    moved = DT.augment_patches(dev, others, ps, True)
    assert torch.equal(_bits(moved[2]), _bits(got[2]))
    assert all(not torch.equal(moved[b], got[b]) for b in (0, 1, 3))


# ---- chunking ----------------------------------------------------------------------------------------------------------------------

def test_chunks_slice_every_array_with_the_images():
    from detectinblur_amd.models import deblur_train as DT
    B = DT.PATCH_MAX_BATCH + 1
    g = torch.Generator().manual_seed(3)
    images = [torch.rand(3, 4, 4, generator=g).cuda() for _ in range(B)]
    draws = [draws_of(b % 8, ((0, 1, 2), (2, 1, 0), (1, 0, 2))[b % 3], saturation=0.5 + b / B, sigma=1.0 + 0.1 * b, key=(b, 2 * b + 1))
             for b in range(B)]
    got = DT.augment_patches(images, draws, 4, True)
    assert got.shape == (B, 3, 4, 4)
    for b in (0, 1, 62, 63, 64):
        assert torch.equal(_bits(got[b]), _bits(DT.augment_patches([images[b]], [draws[b]], 4, True)[0])), b
    singles = torch.cat([DT.augment_patches([images[b]], [draws[b]], 4, True) for b in range(2, 62)])
    assert torch.equal(_bits(got[2:62]), _bits(singles))


# ---- identity through the pyramid kernels --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("levels_dtype", [torch.float32, torch.float16], ids=["pyramid", "pyramid_f16"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_identity_through_the_pyramid_kernels(dtype, levels_dtype):
    from detectinblur_amd.models import deblur_train as DT
    images = [special_image(dtype, 0).cuda(), special_image(dtype, 1).cuda()]
    for bits in (0, 3, 5, 6):
        draws = [draws_of(bits, (2, 0, 1), 4, 0, sigma=2.0, key=(1, 2)), draws_of(bits, (0, 1, 2), 1, 3)]
        got = DT.patch_levels(DT.augment_patches(images, draws, 16, False), 2, levels_dtype)
        want = DT.patch_levels(DT.gather_patches(images, draws, 16), 2, levels_dtype)
        for a, b in zip(got, want):
            assert a.dtype == levels_dtype and torch.equal(a[:, :3], b[:, :3]) and torch.isfinite(a[:, :3]).all(), bits


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_argument_errors_launch_nothing():
    from detectinblur_amd import _lib
    from detectinblur_amd.models import deblur_train as DT
    images = [torch.zeros(3, 12, 12, device="cuda")]
    with pytest.raises(_lib.DibError, match="leaves the"):
        DT.augment_patches(images, [DT.PatchDraw(1, 0, False, False, False, (0, 1, 2))], 12, True)
    with pytest.raises(_lib.DibError, match="flags"):
        DT.augment_patches(images, [DT.PatchDraw(0, 0, False, False, False, (0, 1, 3))], 12, True)
    with pytest.raises(_lib.DibError, match="saturation"):
        DT.augment_patches(images, [DT.PatchDraw(0, 0, False, False, False, (0, 1, 2), -1.0)], 12, True)
    with pytest.raises(_lib.DibError, match="sigma"):
        DT.augment_patches(images, [DT.PatchDraw(0, 0, False, False, False, (0, 1, 2), 1.0, float("inf"))], 12, True)
    torch.cuda.synchronize()
    assert _lib.lib().dib_device_status(0) == 0


# ---- the driver --------------------------------------------------------------------------------------------------------------------

FLAGS = ["--change_saturation", "--patch_noise_sigma", "2"]


def _drive(out_dir, *extra):
    """One driver run on the HIP path, under torch.backends.cudnn.deterministic: without that switch MIOpen's convolution backward does
    not repeat from run to run -- two runs of the trainer from one seed on an MI355X, WITHOUT either flag, the step as it was before them,
    gave the same input and target levels, the same first-step outputs and loss, and then second-step outputs that differ and 13 of 26
    weight tensors that differ by up to 1.9e-7 (7.5e-9 with the flags); with the switch every checksum and every weight was equal, with
    and without the flags.  The patches and their levels were bit-identical in all eight runs: what this file checks repeats exactly."""
    from detectinblur_amd import train_deblurrer as TD
    from detectinblur_amd.models import deblur_train as DT
    saved = DT.FUSE_DEBLUR_TRAIN, DT.FUSE_DEBLUR_TRAIN_AMP, torch.backends.cudnn.deterministic
    buf = io.StringIO()
    try:
        DT.FUSE_DEBLUR_TRAIN = DT.FUSE_DEBLUR_TRAIN_AMP = True
        torch.backends.cudnn.deterministic = True
        with contextlib.redirect_stdout(buf):
            trainer = TD.main(["--synthetic", "--synthetic_images", "4", "--synthetic_size", "72", "88", "--device", "cuda", "-j", "0", "-b", "2",
                               "--patch_size", "16", "--print_freq", "1", "--param_index", "1", "--output_dir", str(out_dir)] + TINY + FLAGS
                              + list(extra))
    finally:
        DT.FUSE_DEBLUR_TRAIN, DT.FUSE_DEBLUR_TRAIN_AMP, torch.backends.cudnn.deterministic = saved
    return buf.getvalue(), trainer


def _weights(out_dir, epoch):
    return torch.load(out_dir / "models" / ("model-%d.pt" % epoch), map_location="cpu", weights_only=True)["G"]


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
def test_driver_with_both_flags_is_reproducible(tmp_path, amp):
    from detectinblur_amd import _lib
    extra = ["--epochs", "1"] + (["--amp"] if amp else [])
    text, trainer = _drive(tmp_path / "a", *extra)
    _drive(tmp_path / "b", *extra)
    losses = [float(v) for v in re.findall(r"loss: ([0-9.einfa+-]+)", text)]
    assert len(losses) == 2 and all(np.isfinite(losses)), text[-2000:]
    assert trainer.bare.last_path == ("hip-amp" if amp else "hip") and text.count("path: hip-amp" if amp else "path: hip") == 2
    a, b = _weights(tmp_path / "a", 1), _weights(tmp_path / "b", 1)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    torch.cuda.synchronize()
    assert _lib.lib().dib_device_status(0) == 0


def test_resume_with_both_flags_matches_the_uninterrupted_run(tmp_path):
    _drive(tmp_path / "a", "--epochs", "2", "--save_every", "1")
    _drive(tmp_path / "b", "--epochs", "1", "--save_every", "1")
    text, _ = _drive(tmp_path / "b", "--epochs", "2", "--save_every", "1", "--resume")
    assert "Resumed from" in text and "Epoch: [2]" in text and "Epoch: [1]" not in text
    a, b, first = _weights(tmp_path / "a", 2), _weights(tmp_path / "b", 2), _weights(tmp_path / "a", 1)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(a[k], first[k]) for k in a)
