"""DeepDeblur's saturation change and add_noise in the trainer (--change_saturation, --patch_noise_sigma) without a GPU: the closed form
of models/deblur_train.augment_patches_torch against a literal float64 restatement of scikit-image's rgb2hsv / hsv2rgb (scikit-image is
not a dependency: the formulae are cited below), the identity at saturation 1 without noise, the grey-level round trip, the draw order
against the reference's dataCommon.py (restated with line numbers), the driver on the CPU, and the entry point's refusals."""
import contextlib
import ctypes
import io
import random
import re

import numpy as np
import pytest
import torch

from detectinblur_amd import train_deblurrer as TD
from detectinblur_amd.models import deblur
from detectinblur_amd.models import deblur_train as DT
from tests.test_deblur_train import TINY, _datacommon_draws

FACTORS = (0.5, 0.77, 1.0, 1.23, 1.5)
# |fp32 closed form - float64 HSV round trip| in grey levels: three fp32 operations (m - q is exact; the product, the difference, and
# with noise the sum) on values of at most 1.5 * 255, each within 2^-24 relative: under 1e-4.  Measured on the CPU: 2.9e-5.
TOL = 1e-3


# ---- scikit-image's colour conversions, restated in float64 ------------------------------------------------------------------------

def rgb2hsv64(rgb):
    """skimage.color.rgb2hsv (skimage/color/colorconv.py) on a float64 [..., 3] array in 0..1, statement for statement."""
    arr = np.asarray(rgb, dtype=np.float64)
    out = np.zeros_like(arr)
    out_v = arr.max(-1)                                            # V
    delta = np.ptp(arr, -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        out_s = delta / out_v                                      # S
        out_s[delta == 0.0] = 0.0
        idx = arr[..., 0] == out_v                                 # red is max
        out[idx, 0] = (arr[idx, 1] - arr[idx, 2]) / delta[idx]
        idx = arr[..., 1] == out_v                                 # green is max
        out[idx, 0] = 2.0 + (arr[idx, 2] - arr[idx, 0]) / delta[idx]
        idx = arr[..., 2] == out_v                                 # blue is max
        out[idx, 0] = 4.0 + (arr[idx, 0] - arr[idx, 1]) / delta[idx]
        out_h = (out[..., 0] / 6.0) % 1.0
    out_h[delta == 0.0] = 0.0
    out[..., 0], out[..., 1], out[..., 2] = out_h, out_s, out_v
    out[np.isnan(out)] = 0
    return out


def hsv2rgb64(hsv):
    """skimage.color.hsv2rgb: the six-sector `choose`."""
    arr = np.asarray(hsv, dtype=np.float64)
    hi = np.floor(arr[..., 0] * 6)
    f = arr[..., 0] * 6 - hi
    v = arr[..., 2]
    p = v * (1 - arr[..., 1])
    q = v * (1 - f * arr[..., 1])
    t = v * (1 - (1 - f) * arr[..., 1])
    hi = np.stack([hi, hi, hi], axis=-1).astype(np.uint8) % 6
    return np.choose(hi, np.stack([np.stack((v, t, p), axis=-1), np.stack((q, v, p), axis=-1), np.stack((p, v, t), axis=-1),
                                   np.stack((p, q, v), axis=-1), np.stack((t, p, v), axis=-1), np.stack((v, p, q), axis=-1)]))


def saturation64(levels, a):
    """dataCommon.py:83-87 on the 8-bit levels of a planar [3, h, w] array: hsv2rgb(rgb2hsv(img) with S *= a).clip(0, 1) * 255, in
    float64 (rgb2hsv scales a uint8 image by 1 / 255), planar again."""
    img = np.moveaxis(np.asarray(levels, dtype=np.float64), 0, -1) / 255.0
    hsv = rgb2hsv64(img)
    hsv[..., 1] *= np.float64(np.float32(a))
    return np.moveaxis(hsv2rgb64(hsv).clip(0, 1) * 255.0, -1, 0)


# ---- the test images ---------------------------------------------------------------------------------------------------------------

GRID_PS = 33


def colour_grid_levels():
    """The 33^3 grid of levels {0, 8, ..., 248, 255} per channel as a [3, 33, 1089] array, and [3, 33, 99] of greys, of black and of
    two-channel ties at the maximum: both are covered by 33 x 33 patches, 36 in all."""
    lv = np.array(list(range(0, 256, 8)) + [255], dtype=np.float32)
    r, g, b = np.meshgrid(lv, lv, lv, indexing="ij")
    grid = np.stack([r.reshape(33, 1089), g.reshape(33, 1089), b.reshape(33, 1089)])
    k = np.arange(33 * 33, dtype=np.int64).reshape(33, 33)
    grey = np.broadcast_to(((k * 7) % 256).astype(np.float32), (3, 33, 33))
    black = np.zeros((3, 33, 33), dtype=np.float32)
    top, low = ((k * 5) % 255 + 1).astype(np.float32), ((k * 3) % 256).astype(np.float32)
    low = np.minimum(low, top)
    ties = np.stack([top, top, low])
    ties[:, 11:22] = np.stack([low, top, top])[:, 11:22]
    ties[:, 22:] = np.stack([top, low, top])[:, 22:]
    return grid, np.concatenate([grey, black, ties], axis=2)


def grid_patches(dtype=torch.float32):
    """-> (images, origins): the two arrays above as level / 255 images of `dtype`, and the (image index, px) of the 36 patches."""
    arrays = colour_grid_levels()
    images = [(torch.from_numpy(np.ascontiguousarray(a)) / 255.0).to(dtype) for a in arrays]
    origins = [(i, px) for i, a in enumerate(arrays) for px in range(0, a.shape[2], GRID_PS)]
    return images, origins


def special_image(dtype, seed=0):
    """[3, 20, 20]: every 8-bit level / 255, NaN, +-inf, negatives, values above 1, -0.0 and values between the levels."""
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(1200, generator=g) * 1.5 - 0.25
    v[:256] = torch.arange(256, dtype=torch.float32) / 255.0
    v[256:264] = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, -1.0, 1.0001, 2.5, 1e-8])
    return v[torch.randperm(1200, generator=g)].reshape(3, 20, 20).to(dtype)


def draws_of(bits, order, py=0, px=0, **kw):
    return DT.PatchDraw(py, px, bool(bits & 1), bool(bits & 2), bool(bits & 4), order, **kw)


# ---- the closed form ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a", FACTORS)
def test_closed_form_against_the_float64_hsv_round_trip(a):
    images, origins = grid_patches()
    ims = [images[i] for i, _ in origins]
    draws = [draws_of(0, (0, 1, 2), 0, px, saturation=a) for _, px in origins]
    x = DT.augment_patches_torch(ims, draws, GRID_PS, True, pre_rounding=True).double().numpy()
    g = DT.augment_patches_torch(ims, draws, GRID_PS, True).numpy()
    assert x.shape == g.shape == (36, 3, 33, 33) and g.dtype == np.float32
    levels = np.rint(g.astype(np.float64) * 255.0)
    assert np.array_equal((levels / 255.0).astype(np.float32), g)                       # grey levels / 255, nothing else
    arrays = colour_grid_levels()
    want = np.stack([saturation64(arrays[i][:, :, px:px + GRID_PS], a) for i, px in origins])
    err = np.abs(x - want)
    print("a = %g: max |fp32 closed form - float64 HSV| = %.3g grey levels" % (a, err.max()))
    assert (err <= TOL).all(), float(err.max())
    assert (np.abs(levels - want) <= 0.5 + TOL).all(), float(np.abs(levels - want).max())
    if a == 1.0:
        assert np.array_equal(levels, np.stack([arrays[i][:, :, px:px + GRID_PS] for i, px in origins]))


def test_grey_level_round_trip():
    g = torch.arange(256, dtype=torch.float32)
    stored = g / torch.full((), 255.0)
    assert stored.dtype == torch.float32 and torch.equal(deblur.quantise(stored.reshape(1, 16, 16)).reshape(-1), g)


# ---- identity ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_saturation_one_without_noise_gives_the_plain_levels(dtype):
    images = [special_image(dtype, 0), special_image(dtype, 1)]
    for order in ((2, 0, 1), (0, 1, 2)):
        for bits in range(8):
            # a sigma and a key that `noise=False` must ignore
            draws = [draws_of(bits, order, 4, 0), draws_of(bits, order, 1, 3, sigma=3.0, key=(5, 6))]
            got = DT.patch_levels(DT.augment_patches_torch(images, draws, 16, False), 2)
            want = DT.patch_levels(DT.gather_patches_torch(images, draws, 16), 2)
            for a, b in zip(got, want):
                assert torch.equal(a[:, :3].contiguous().view(torch.int32), b[:, :3].contiguous().view(torch.int32)), (order, bits)


def test_cpu_noise_is_reproducible_clipped_and_on_the_input_only():
    images = [special_image(torch.float32, 2)]
    d = draws_of(3, (1, 2, 0), 2, 2, saturation=1.3, sigma=-4.0, key=(123, 456))
    a, b = DT.augment_patches(images, [d], 16, True), DT.augment_patches(images, [d], 16, True)
    clean = DT.augment_patches(images, [d], 16, False)
    assert torch.equal(a, b) and not torch.equal(a, clean)
    assert torch.equal(clean, DT.augment_patches(images, [d._replace(sigma=0.0)], 16, True))
    lv = a * 255
    assert torch.equal(lv.round(), lv.round().clamp(0, 255)) and (lv - lv.round()).abs().max() < 1e-4
    assert not torch.equal(a, DT.augment_patches(images, [d._replace(key=(123, 457))], 16, True))
    resid = (a - clean)[(clean > 0.2) & (clean < 0.8)] * 255          # away from the clip: sigma n, rounded to levels
    assert 3.0 < float(resid.std()) < 5.0 and abs(float(resid.mean())) < 1.0


# ---- draws -------------------------------------------------------------------------------------------------------------------------

def _datacommon_value_draws(sigma_sigma, rgb_range=255):
    amp_factor = np.random.uniform(0.5, 1.5)                                    # augment :73
    sigma = np.random.normal() * sigma_sigma * rgb_range / 255                 # add_noise :48
    key = np.random.randint(0, 2 ** 32, size=2, dtype=np.uint32)               # in place of the randn field of :51
    return amp_factor, sigma, (int(key[0]), int(key[1]))


@pytest.mark.parametrize("seed", [0, 7, 1337])
def test_draws_off_are_the_six_and_touch_no_numpy_state(seed):
    random.seed(seed)
    np.random.seed(seed)
    want = _datacommon_draws(40, 56, 16)
    after = random.random()
    random.seed(seed)
    before = np.random.get_state()
    got = DT.draw_patch(40, 56, 16)
    assert random.random() == after
    now = np.random.get_state()
    assert before[0] == now[0] and np.array_equal(before[1], now[1]) and before[2:] == now[2:]
    assert (got.py, got.px, got.hflip, got.vflip, got.rot90, list(got.order)) == want
    assert tuple(got) == want[:5] + (tuple(want[5]), 1.0, 0.0, (0, 0))
    assert DT.PatchDraw(1, 2, False, True, False, (0, 1, 2)) == (1, 2, False, True, False, (0, 1, 2), 1.0, 0.0, (0, 0))


@pytest.mark.parametrize("seed", [0, 7, 1337])
def test_draws_on_follow_datacommons_order(seed):
    random.seed(seed)
    np.random.seed(seed)
    want = [(_datacommon_draws(40, 56, 16), _datacommon_value_draws(2.0)) for _ in range(2)]
    after = random.random(), np.random.random_sample()
    random.seed(seed)
    np.random.seed(seed)
    got = [DT.draw_patch(40, 56, 16, True, 2.0) for _ in range(2)]
    assert (random.random(), np.random.random_sample()) == after
    for (six, (a, s, key)), g in zip(want, got):
        assert (g.py, g.px, g.hflip, g.vflip, g.rot90, list(g.order)) == six
        assert (g.saturation, g.sigma, g.key) == (a, s, key)
        assert 0.5 <= g.saturation < 1.5 and all(0 <= k < 2 ** 32 for k in g.key)
    # each option alone takes its own draws only
    np.random.seed(seed)
    a = np.random.uniform(0.5, 1.5)
    np.random.seed(seed)
    g = DT.draw_patch(40, 56, 16, True, 0.0)
    assert (g.saturation, g.sigma, g.key) == (a, 0.0, (0, 0))
    np.random.seed(seed)
    s = np.random.normal() * 2.0
    np.random.seed(seed)
    g = DT.draw_patch(40, 56, 16, False, 2.0)
    assert (g.saturation, g.sigma) == (1.0, s) and g.key != (0, 0)


# ---- the driver --------------------------------------------------------------------------------------------------------------------

def test_refusals_and_defaults():
    with pytest.raises(SystemExit, match="patch_noise_sigma"):
        TD.main(["--synthetic", "--patch_noise_sigma", "-1"])
    with pytest.raises(SystemExit, match="patch_noise_sigma"):
        TD.main(["--synthetic", "--patch_noise_sigma", "nan"])
    with pytest.raises(SystemExit, match="patch_noise_sigma"):
        TD.main(["--synthetic", "--patch_noise_sigma", "inf"])
    args = TD.build_parser().parse_args(["--synthetic"])
    assert args.change_saturation is False and args.patch_noise_sigma == 0.0
    assert args.add_noise is False and args.noise_level == 0.001               # the blur stage's own flags are what they were
    TD.reject(args)


def _run(out_dir, *extra):
    argv = ["--synthetic", "--synthetic_images", "4", "--synthetic_size", "40", "56", "--device", "cpu", "-j", "0", "-b", "2",
            "--patch_size", "16", "--print_freq", "1", "--epochs", "1", "--output_dir", str(out_dir)] + TINY + list(extra)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        TD.main(argv)
    return buf.getvalue()


def test_driver_on_the_cpu_is_reproducible_with_both_flags(tmp_path):
    flags = ("--change_saturation", "--patch_noise_sigma", "2")
    text = _run(tmp_path / "a", *flags)
    _run(tmp_path / "b", *flags)
    _run(tmp_path / "plain")
    losses = [float(v) for v in re.findall(r"loss: ([0-9.einfa+-]+)", text)]
    assert len(losses) == 2 and all(np.isfinite(losses)), text[-2000:]
    a, b, plain = (torch.load(tmp_path / d / "models" / "model-1.pt", weights_only=True)["G"] for d in ("a", "b", "plain"))
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(a[k], plain[k]) for k in a)                     # the flags did change the pairs


# ---- the entry point's refusals, without a GPU ---------------------------------------------------------------------------------------

def _call(saturation=1.0, sigma=0.0, in_ptr=0x1000, out_ptr=0x2000, py=0, flags=0x240):
    from detectinblur_amd import _lib
    l = _lib.lib()
    one = lambda t, v: (t * 1)(v)          # noqa: E731
    code = l.dib_deblur_patches_augment(_lib.ptr_array([in_ptr]), _lib.DIB_F32, _lib.int_array([12]), _lib.int_array([12]), _lib.int_array([py]),
                                        _lib.int_array([0]), one(ctypes.c_uint, flags), one(ctypes.c_float, saturation),
                                        one(ctypes.c_float, sigma), (ctypes.c_uint * 2)(1, 2), 1, 12, out_ptr, None)
    return code, l.dib_last_error().decode()


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Every case returns before the launch: the pointers are never read, and no GPU is needed."""
    from detectinblur_amd import _lib
    for bad in (float("nan"), float("inf"), -0.5):
        code, text = _call(saturation=bad)
        assert code == _lib.DIB_EINVAL and "saturation" in text and "dib_deblur_patches_augment" in text, (bad, text)
    for bad in (float("nan"), float("-inf")):
        code, text = _call(sigma=bad)
        assert code == _lib.DIB_EINVAL and "sigma" in text, (bad, text)
    code, text = _call(in_ptr=None)
    assert code == _lib.DIB_EINVAL and "null" in text
    code, text = _call(out_ptr=None)
    assert code == _lib.DIB_EINVAL and "null pointer" in text
    code, text = _call(out_ptr=0x2002)
    assert code == _lib.DIB_EINVAL and "4-byte aligned" in text
    code, text = _call(py=1)
    assert code == _lib.DIB_ESHAPE and "leaves the" in text
    code, text = _call(flags=0x2C0)
    assert code == _lib.DIB_EINVAL and "flags" in text
    l = _lib.lib()
    assert l.dib_deblur_patches_augment(None, _lib.DIB_F32, None, None, None, None, None, None, None, None, 65, 12, None, None) == _lib.DIB_EINVAL
    assert b"B <= 64" in l.dib_last_error()
